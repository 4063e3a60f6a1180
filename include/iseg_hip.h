/* iseg_hip.h -- C ABI of libiseg_hip.so, the MI355X (gfx950) compute library behind iseg_amd.
 *
 * The reference (edwardyehuang/iSeg) has no native boundary: its "kernels" are TensorFlow/Keras ops reached
 * through Python call signatures.  Each entry point below therefore cites the reference Python call site(s)
 * whose per-step arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - C linkage, plain pointers and sizes; no torch / C++ types.
 *   - Pointers are DEVICE pointers unless the name ends in _h. Tensors are dense NHWC / row-major.
 *   - dtype: ISEG_F32 (0) or ISEG_BF16 (1) storage; arithmetic is fp32 (MFMA accumulates in fp32).
 *   - Returns ISEG_OK (0) or a negative iseg status; iseg_last_error() holds a per-thread message.
 *   - Nothing allocates or frees device memory: the caller owns inputs, outputs and workspace
 *     (query iseg_*_workspace_bytes first).  An entry point that is handed fewer workspace bytes than
 *     its query answers returns ISEG_STATUS_WORKSPACE and launches nothing (a NULL workspace where one
 *     is needed: ISEG_STATUS_WORKSPACE or ISEG_STATUS_ARG); the answer may be an upper bound over the
 *     routes an entry point can take, and it is the answer that is checked.  All work is
 *     enqueued on `stream`; entry points never synchronise, so they can be captured into a hipGraph.
 *   - Keras weight layouts are consumed as they are: Dense [in,out], Conv2D [kh,kw,Cin,Cout],
 *     DepthwiseConv2D [kh,kw,C,1].
 */
#ifndef ISEG_HIP_H
#define ISEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef ISEG_HIP_STREAM_T
#define ISEG_HIP_STREAM_T
typedef struct ihipStream_t* iseg_stream_t; /* == hipStream_t */
#endif

#define ISEG_STATUS_OK 0
#define ISEG_STATUS_ARG (-1)
#define ISEG_STATUS_HIP (-2)
#define ISEG_STATUS_UNSUPPORTED (-3)
#define ISEG_STATUS_WORKSPACE (-4)

#define ISEG_DTYPE_F32 0
#define ISEG_DTYPE_BF16 1

/* epilogue activations of iseg_gemm */
#define ISEG_ACT_NONE 0
#define ISEG_ACT_RELU 1      /* keras.activations.relu   (layers/model_builder.py:66,92-93) */
#define ISEG_ACT_GELU 2      /* keras.activations.gelu, exact erf (backbones/convnext.py:53) */
#define ISEG_ACT_GELU_GRAD 3 /* v *= gelu'(aux)  : backward of ISEG_ACT_GELU, aux = saved pre-activation */
#define ISEG_ACT_RELU_GRAD 4 /* v  = aux > 0 ? v : 0 */
#define ISEG_ACT_MUL_AUX 5   /* v *= aux : backward of ISEG_ACT_GELU when the forward saved gelu'(pre) (pre_deriv = 1) */
#define ISEG_ACT_SIGMOID 6   /* tf.nn.sigmoid (layers/nasfpn.py:304-311 global-attention gate); iseg_act_fwd / iseg_act_bwd only */
#define ISEG_ACT_SWISH 7     /* tf.nn.silu / keras "swish": x sigmoid(x) (backbones/eva/swiglu.py:13, layers/nasfpn.py:289); iseg_act_fwd / _bwd only */
#define ISEG_ACT_GELU_TANH 8 /* keras.activations.gelu(approximate=True): 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) (nlp/gemma/gemma_decoder_block.py:167-170); iseg_act_* / iseg_glu_* only */

int iseg_version(void);
/* copies the calling thread's last error message (NUL-terminated) into buf_h; returns its length */
size_t iseg_last_error(char* buf_h, size_t n);

/* ---------------------------------------------------------------------------------------------------------
 * Dense contraction  D[M,N] = epilogue( alpha * sum_k A(m,k) B(k,n) )
 * Replaces: keras.layers.Dense (backbones/convnext.py:29-30,51-54; backbones/swin.py Mlp/qkv/proj;
 * backbones/vit.py MLPBlock), 1x1 keras.layers.Conv2D (layers/model_builder.py:54-64; layers/core_model_ext.py:129)
 * and, after iseg_im2col, every spatial Conv2D (layers/aspp.py:41-52; backbones/convnext.py:72-75), plus their
 * autodiff transposes (dgrad: a_kcontig=1,b_kcontig=1 on the Keras kernel as stored; wgrad: a_kcontig=0,b_kcontig=0).
 *   a_kcontig=1: A(m,k) = A[m*lda + k]      a_kcontig=0: A(m,k) = A[k*lda + m]
 *   b_kcontig=1: B(k,n) = B[n*ldb + k]      b_kcontig=0: B(k,n) = B[k*ldb + n]   (Keras [in,out])
 * Epilogue, in this order:  v = alpha*acc ; v += bias[n] ; pre_out[m,n] = v (or gelu'(v), pre_deriv) ; act ; v *= colscale[n] ;
 *   v *= rowscale[m / rows_per_group] ; v += residual[m,n] ; v += D[m,n] if accumulate ; D[m,n] = v.
 * residual / aux / pre_out have the OUTPUT dtype.  in_dtype bf16 -> MFMA path; f32 -> fp32 FMA (parity) path.
 * split_k: 0 = automatic (skinny outputs with a long reduction are split and reduced in slab order:
 * deterministic), n>0 = forced.  Workspace: iseg_gemm_workspace_bytes().
 * --------------------------------------------------------------------------------------------------------- */
typedef struct iseg_gemm_args {
    const void* A;
    int64_t lda;
    int a_kcontig;
    const void* B;
    int64_t ldb;
    int b_kcontig;
    void* D;
    int64_t ldd;
    int64_t M, N, K;
    int in_dtype, out_dtype;
    const float* bias;     /* [N] or NULL */
    const float* colscale; /* [N] or NULL  (ConvNeXt layer scale gamma, backbones/convnext.py:56-57) */
    const float* rowscale; /* [ceil(M/rows_per_group)] or NULL (drop_path per-sample factor, utils/drops.py:8-22) */
    int64_t rows_per_group;
    const void* residual; /* [M, ldr] or NULL */
    int64_t ldr;
    const void* aux; /* [M, ldaux], needed by ISEG_ACT_*_GRAD and ISEG_ACT_MUL_AUX */
    int64_t ldaux;
    void* pre_out; /* [M, ldp] or NULL: pre-activation saved for backward */
    int64_t ldp;
    int act;
    float alpha;
    int accumulate;
    int split_k;
    int a_act; /* ISEG_ACT_NONE or ISEG_ACT_GELU: A := gelu(A) applied while the operand is staged (the GELU output of
                  backbones/convnext.py:53 is never materialised; pwconv2 and its weight gradient re-derive it) */
    float* colsum_out; /* [N] or NULL.  wgrad orientation only (a_kcontig=0,b_kcontig=0, bf16, M % 8 == 0): also returns
                          sum_k B(k,:) -- the Dense bias gradient -- from a virtual ones-row of A, i.e. without another pass
                          over the [pixels, N] gradient tensor */
    int colsum_accumulate;
    int defer_reduce; /* 1: a split-K problem only writes its slabs; the caller finishes with iseg_gemm_reduce (lets the two
                         kernels be timed / scheduled separately) */
    /* strided batch (attention: one problem per (sample, head)); batch <= 1 = a single problem.  Problem z reads/writes at
       X + (z / batch_inner) * sX_outer + (z % batch_inner) * sX_inner (elements).  Batched problems take only the
       alpha / accumulate epilogue and are never split along K. */
    int batch, batch_inner;
    int64_t sa_outer, sa_inner, sb_outer, sb_inner, sd_outer, sd_inner;
    int pre_deriv; /* 1 (needs act = ISEG_ACT_GELU and pre_out): pre_out receives gelu'(pre-activation) instead of the pre-activation --
                      the forward epilogue has Phi(v) and exp(-v^2/2) in hand anyway, and the backward GEMM's epilogue becomes one
                      multiply (ISEG_ACT_MUL_AUX) instead of re-evaluating erf per element (50 us of VALU per 100 M elements) */
    /* B per row group (b_group_rows > 0): rows [i*b_group_rows, (i+1)*b_group_rows) of A / D are multiplied by B + i*b_group_stride
       (elements) -- one kernel per sample, e.g. the Dense after ConvNeXt V2's response normalisation with the per-sample channel factors
       folded into its kernel (backbones/convnext_v2.py:92-93).  Every epilogue option stays available (rows keep their global index).
       bf16, both operands K-contiguous, b_group_rows % 256 == 0, no split-K, no batch; anything else returns ISEG_ERR_UNSUPPORTED. */
    int64_t b_group_rows, b_group_stride;
} iseg_gemm_args;

int iseg_gemm_splits(const iseg_gemm_args* args_h);
/* slabs a deferred split problem really writes ([slab][M (+1 with colsum_out)][N] fp32 in the workspace): <= iseg_gemm_splits, the K range is cut
 * into multiples of 128 -- for a consumer that sums the slabs itself (iseg_layerscale_grads_slabs) */
int iseg_gemm_slabs(const iseg_gemm_args* args_h);
/* which main loop iseg_gemm runs for this problem (profiling labels): 0 = register-staged gemm_bf16_kernel / fp32 kernel,
   K-contiguous A and B on the LDS-DMA pipeline gemm_bf16_dma_kernel: 1 = 128x64 tiles, 2 = 256x128, 4 = 128x128 (3 stages), 6 = 256x192
   (2 stages), 8 = 128x192, 9 = 64x192 (3 and 5 are unused: 128x128 with 2 stages could not be planned, a persistent 256x128 form was dropped),
   7 / 8 = the weight-gradient orientation (a_kcontig = b_kcontig = 0, split over K: Dense / 1x1-conv kernel gradients,
   layers' `kernel` of backbones/convnext.py:51-55, backbones/swin.py:17-43) on the LDS-DMA pipeline gemm_bf16_dma_tn_kernel with
   256x128 / 128x256 tiles (M, N multiples of 8 and >= 128 -- or one of them 64..127 when the other is >= 320 --, any K >= 2048, aligned operands) */
int iseg_gemm_variant(const iseg_gemm_args* args_h);
size_t iseg_gemm_workspace_bytes(const iseg_gemm_args* args_h);
int iseg_gemm(const iseg_gemm_args* args_h, void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_gemm_reduce(const iseg_gemm_args* args_h, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* Two weight-gradient problems over the SAME reduction rows in one launch (the pair of an un-fused ConvNeXt block's backward pass,
 * backbones/convnext.py:51-54: Z = gelu(h)^T dout and dW1 = y2^T dH).  iseg_gemm_tn_pair_splits: the common split count, 0 = run them one by one.
 * The caller sets split_k to it in both blocks; iseg_gemm_tn_pair writes both problems' slabs (as defer_reduce = 1 does) and each problem is
 * finished by iseg_gemm_reduce or by a consumer of its slabs (iseg_layerscale_grads_slabs). */
int iseg_gemm_tn_pair_splits(const iseg_gemm_args* g0, const iseg_gemm_args* g1);
int iseg_gemm_tn_pair(const iseg_gemm_args* g0, void* ws0, size_t ws0_bytes, const iseg_gemm_args* g1, void* ws1, size_t ws1_bytes,
                      iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * LayerNorm over the last axis: keras.layers.LayerNormalization(axis=-1, epsilon)
 * (backbones/convnext.py:27,71; backbones/swin.py norm1/norm2; backbones/vit.py). x,y: [rows, C].  C % 8 == 0 takes the 16-byte-vector kernels;
 * any other C (<= 4096 for the backward; EVA02-large's 2730 hidden units, backbones/eva/swiglu.py:74-80) a one-wavefront-per-row form -- plain
 * iseg_layernorm_fwd / _bwd only, not the gather / post-norm entry points.
 * mean/rstd [rows] are saved for the backward.  bwd: dx (= dx_add + LN^T dy), dgamma, dbeta.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int64_t rows,
                       int C, float eps, int dtype, iseg_stream_t stream);
size_t iseg_layernorm_bwd_workspace_bytes(int64_t rows, int C);
int iseg_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                       const void* dx_add, float* dgamma, float* dbeta, int accumulate_param_grads, int64_t rows, int C,
                       int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* Tail of a post-norm residual branch in one pass each way (backbones/intern_image/intern_image.py:226-236: x = residual + drop_path(gamma *
 * norm(f(x))), utils/drops.py:8-22): y = residual + rowscale[row / rows_per_group] * colscale[c] * LN(x); colscale [C], rowscale, residual
 * optional.  Backward: dx = LN^T(rowscale colscale dy); dgamma, dbeta and dcolscale (NULL: not wanted) are ACCUMULATED -- the three come from
 * the same two column sums.  Workspace of the backward: iseg_layernorm_bwd_workspace_bytes(rows, C) + 2 C floats, with or without a scale. */
int iseg_layernorm_post_fwd(const void* x, const float* gamma, const float* beta, const float* colscale, const float* rowscale,
                            int64_t rows_per_group, const void* residual, void* y, float* mean, float* rstd, int64_t rows, int C, float eps,
                            int dtype, iseg_stream_t stream);
int iseg_layernorm_post_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* colscale, const float* rowscale,
                            int64_t rows_per_group, const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                            float* dcolscale, int64_t rows, int C, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* LayerNorm followed by a static row permutation with zero padding -- norm1 + tf.pad + tf.roll + window_partition of a Swin block
 * (backbones/swin.py:246-262) in one pass: y[r,:] = src_index[r] >= 0 ? LN(x[src_index[r],:]) : 0 for r < rows_out; mean / rstd [rows_out]
 * are kept per OUTPUT row.  Backward over the `rows` SOURCE rows with the inverse table: the gradient row and the statistics of source row
 * r sit at row dy_index[r] (< 0: no gradient arrives); dx = dx_add + LN^T dy as in iseg_layernorm_bwd (same workspace). */
int iseg_layernorm_gather_fwd(const void* x, const int32_t* src_index, const float* gamma, const float* beta, void* y, float* mean,
                              float* rstd, int64_t rows_out, int C, float eps, int dtype, iseg_stream_t stream);
int iseg_layernorm_gather_bwd(const void* dy, const int32_t* dy_index, const void* x, const float* gamma, const float* mean,
                              const float* rstd, void* dx, const void* dx_add, float* dgamma, float* dbeta, int accumulate_param_grads,
                              int64_t rows, int C, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Depthwise KxK conv, stride 1, dilation `dil`, explicit top/left padding (TF "same": pad = (K-1)*dil/2):
 * keras.layers.DepthwiseConv2D (backbones/convnext.py:25,50; build_dilated_convnext :245-266).
 * w: [K*K, C] fp32 (the Keras [K,K,C,1] kernel), bias [C] or NULL.  y = conv(x) + bias (+ add).
 * flip=1 turns it into the data gradient: call with dy as x, pad' = (K-1)*dil - pad, bias NULL, and
 * `add` = gradient arriving through the residual branch.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_dwconv2d_fwd(const void* x, const float* w, const float* bias, const void* add, void* y, int N, int H, int W, int C,
                      int K, int dil, int pad_t, int pad_l, int flip, int dtype, iseg_stream_t stream);
/* The 7 x 7 / bf16 / C % 32 == 0 case of iseg_dwconv2d_fwd on the matrix cores (csrc/dwconv_mfma.hip: banded products with
 * v_mfma_f32_4x4x4_16b_bf16, block = channel) -- the route iseg_dwconv2d_fwd takes by itself for large planes, exported so that
 * tests and benchmarks can take it whenever the shape is eligible.  Same arguments and semantics (backbones/convnext.py:23-27,47-50); weights are rounded to bf16 as the
 * reference's mixed_bfloat16 policy does.  ISEG_ERR_UNSUPPORTED when the shape is not eligible. */
int iseg_dwconv2d7_mfma(const void* x, const float* w, const float* bias, const void* add, void* y, int N, int H, int W, int C, int pad_t,
                        int pad_l, int flip, iseg_stream_t stream);
size_t iseg_dwconv2d_bwd_weight_workspace_bytes(int N, int H, int W, int C, int K);
/* The 7 x 7 weight gradient on the matrix cores (csrc/dwconv_wgrad_mfma.hip), named explicitly: bf16 storage, C % 32 == 0, stride 1, dilation 1.
 * iseg_dwconv2d_bwd_weight takes this route by itself where it measured faster; the workspace size is the same query (K = 7). */
int iseg_dwconv2d7_bwd_weight_mfma(const void* x, const void* dy, float* dw, float* db, int accumulate, int N, int H, int W, int C, int pad_t,
                                   int pad_l, void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_dwconv2d_bwd_weight(const void* x, const void* dy, float* dw, float* db, int accumulate, int N, int H, int W, int C,
                             int K, int dil, int pad_t, int pad_l, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* The same layer with strides = s (backbones/mobilenetv2.py:60-78 the 3x3 / s2 of an inverted residual block; the strided SepConvBnReLU of
 * layers/model_builder.py), computed at the strided output positions only.  pad_t / pad_l: TF "same" front padding for (H, K, s, dil);
 * Ho = ceil(H / s), Wo = ceil(W / s).  The data gradient is the gather over dy (a tap contributes where (h + pad_t - i*dil) is a multiple of
 * s); the weight gradient sums fixed pixel partitions in a fixed order (deterministic) into dw [K*K, C] / db [C] (+= when accumulate). */
int iseg_dwconv2d_strided_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C, int K, int stride, int dil,
                              int pad_t, int pad_l, int Ho, int Wo, int dtype, iseg_stream_t stream);
int iseg_dwconv2d_strided_bwd_data(const void* dy, const float* w, void* dx, int N, int H, int W, int C, int K, int stride, int dil, int pad_t,
                                   int pad_l, int Ho, int Wo, int dtype, iseg_stream_t stream);
size_t iseg_dwconv2d_strided_bwd_weight_workspace_bytes(int N, int Ho, int Wo, int C, int K);
int iseg_dwconv2d_strided_bwd_weight(const void* x, const void* dy, float* dw, float* db, int accumulate, int N, int H, int W, int C, int K,
                                     int stride, int dil, int pad_t, int pad_l, int Ho, int Wo, int dtype, void* ws, size_t ws_bytes,
                                     iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * (Sync)BatchNorm, training mode: keras BatchNormalization(synchronized=True) as wired by
 * layers/normalizations.py:14-23,39-132; moments as layers/keras3/bn.py:10-73 / layers/syncbn.py:70-119.
 *   1. iseg_bn_stats       packed[0:C]=sum x, [C:2C]=sum x^2, [2C]=local count   (one message for RCCL all-reduce)
 *   2. (caller) all-reduce(sum) of packed over ranks
 *   3. iseg_bn_finalize    mean, rstd=rsqrt(var_biased+eps); moving <- moving*momentum + batch*(1-momentum)
 *   4. iseg_bn_apply_fwd   y = act((x-mean)*rstd*gamma+beta); y may be a channel slice (ldy) of a concat buffer
 *  bwd: iseg_bn_bwd_reduce sums[0:C]=sum dz, [C:2C]=sum dz*xhat (dz = dy*relu'(y)); (caller) all-reduce;
 *       iseg_bn_bwd_apply  dx = gamma*rstd*(dz - sums0/n - xhat*sums1/n);  dgamma = sums[C:2C], dbeta = sums[0:C].
 * x: [rows, C] with row stride ldx (elements); C, ld* multiples of 8.
 * --------------------------------------------------------------------------------------------------------- */
size_t iseg_bn_workspace_bytes(int64_t rows, int C);
int iseg_bn_stats(const void* x, int64_t ldx, float* packed, int64_t rows, int C, int dtype, void* ws, size_t ws_bytes,
                  iseg_stream_t stream);
int iseg_bn_finalize(const float* packed, int C, float eps, float momentum, float* mean, float* rstd, float* moving_mean,
                     float* moving_var, iseg_stream_t stream);
int iseg_bn_apply_fwd(const void* x, int64_t ldx, const float* mean, const float* rstd, const float* gamma, const float* beta,
                      void* y, int64_t ldy, int64_t rows, int C, int relu, int dtype, iseg_stream_t stream);
/* iseg_bn_finalize + iseg_bn_apply_fwd in one launch (same arithmetic): mean, rstd [C] are outputs, moving_* updated in place (may be NULL) */
int iseg_bn_apply_fwd_packed(const void* x, int64_t ldx, const float* packed, float eps, float momentum, const float* gamma, const float* beta,
                             float* mean, float* rstd, float* moving_mean, float* moving_var, void* y, int64_t ldy, int64_t rows, int C,
                             int relu, int dtype, iseg_stream_t stream);
int iseg_bn_bwd_reduce(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                       const float* rstd, float* sums, int64_t rows, int C, int relu, int dtype, void* ws, size_t ws_bytes,
                       iseg_stream_t stream);
int iseg_bn_bwd_apply(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                      const float* rstd, const float* gamma, const float* sums, float inv_n, void* dx, int64_t lddx, int64_t rows,
                      int C, int relu, int dtype, iseg_stream_t stream);
/* iseg_bn_bwd_apply that also books the layer's parameter gradients: dbeta += sums[0:C], dgamma += sums[C:2C] (either may be NULL).  Only
 * when `sums` are this replica's own (no all-reduce in between): under data parallelism the gradients are summed over replicas later. */
int iseg_bn_bwd_apply_acc(const void* dy, int64_t lddy, const void* x, int64_t ldx, const void* y, int64_t ldy, const float* mean,
                          const float* rstd, const float* gamma, const float* sums, float inv_n, void* dx, int64_t lddx, float* dgamma,
                          float* dbeta, int64_t rows, int C, int relu, int dtype, iseg_stream_t stream);
/* The fused-ReLU backward pair for a forward that did not keep its output: the ReLU mask is re-derived from x,
 * (x - mean) * rstd * gamma + beta > 0 (the forward's own expression), instead of being read from y. */
int iseg_bn_bwd_reduce_remask(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean, const float* rstd,
                              const float* gamma, const float* beta, float* sums, int64_t rows, int C, int dtype, void* ws, size_t ws_bytes,
                              iseg_stream_t stream);
int iseg_bn_bwd_apply_remask(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* mean, const float* rstd,
                             const float* gamma, const float* beta, const float* sums, float inv_n, void* dx, int64_t lddx, float* dgamma,
                             float* dbeta, int64_t rows, int C, int dtype, iseg_stream_t stream);
/* One level of the FPN top-down pathway (layers/fpn.py:46-57) in one pass: out = relu((z - mean) * rstd * gamma + beta) + bilinear_up(x),
 * TF2 half-pixel bilinear (utils/common.py resize_image); z, out [N, Ho, Wo, C], x [N, Hi, Wi, C], C % 8 == 0.  mean / rstd come from
 * iseg_bn_stats + iseg_bn_finalize; the backward is iseg_resize_bilinear_bwd + the _remask pair above. */
int iseg_bn_relu_upsample_add(const void* z, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* x,
                              void* out, int N, int Hi, int Wi, int Ho, int Wo, int C, int dtype, iseg_stream_t stream);
int iseg_rsqrt_eps(const float* var, float eps, float* out, int n, iseg_stream_t stream); /* inference: rstd of moving var */

/* ---------------------------------------------------------------------------------------------------------
 * EfficientNet MBConv tail (backbones/efficientnet.py:214-255): dwconv_bn -> swish -> squeeze-excite (mean over H*W, se_reduce,
 * swish, se_expand, sigmoid) -> gate, on the depthwise output x [N, HW, C] (NHWC).  z = (x-mean)*rstd*gamma+beta, a = swish(z),
 * m = mean_hw a [N, C], hpre = W1^T m + b1 [N, Cse], g = sigmoid(W2^T swish(hpre) + b2) [N, C], out = a*g; the un-gated a is never
 * stored.  W1 [C, Cse], W2 [Cse, C] (Keras 1x1 kernels), biases and statistics fp32; x / out / dO / dx fp32 or bf16 (dtype).
 * Training statistics: mean / rstd from iseg_bn_stats + (all-reduce) + iseg_bn_finalize; moving statistics: moving_mean and
 * iseg_rsqrt_eps(moving_variance).  Partial sums go to caller-owned buffers and are summed in a fixed order (no float atomics).
 *   fwd: iseg_bn_swish_se_squeeze (x -> partials) ; iseg_se_excite_fwd (partials -> m, hpre, g) ; iseg_bn_swish_gate_fwd (x, g -> out)
 *   bwd: iseg_bn_swish_gate_bwd_reduce (dO, x -> partials of S1 = sum dO*a, S2 = sum dO*s', S3 = sum dO*s'*xhat, S4 = sum s',
 *        S5 = sum s'*xhat per (n, c), s' = swish'(z), xhat = (x-mean)*rstd) ; iseg_se_excite_bwd (-> dW1, db1, dW2, db2 (accumulate
 *        flag; any may be NULL), dmh = dm/HW [N, C], sums [2C] = (sum dz, sum dz*xhat) with dz = (dO*g + dmh)*s': iseg_bn_bwd_reduce's
 *        message layout, (caller) all-reduce) ; iseg_bn_swish_gate_bwd_apply (dx = gamma*rstd*(dz - sums0*inv_n - xhat*sums1*inv_n) when
 *        train, gamma*rstd*dz otherwise; dbeta += sums[0:C], dgamma += sums[C:2C] when non-NULL, only while sums are this replica's own).
 * C % 8 == 0, any HW, any Cse >= 1, (C + Cse) * 4 <= 64 KiB, 16-byte aligned tensors; anything else returns ISEG_ERR_UNSUPPORTED.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_mbconv_supported(int N, int HW, int C, int Cse);
size_t iseg_mbconv_partials_bytes(int N, int HW, int C, int backward);
size_t iseg_se_excite_bwd_workspace_bytes(int N, int C, int Cse);
int iseg_bn_swish_se_squeeze(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* partials,
                             size_t partials_bytes, int N, int HW, int C, int dtype, iseg_stream_t stream);
int iseg_se_excite_fwd(const float* partials, int N, int HW, int C, int Cse, const float* W1, const float* b1, const float* W2, const float* b2,
                       float* m, float* hpre, float* g, iseg_stream_t stream);
int iseg_bn_swish_gate_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const float* g, void* out,
                           int N, int HW, int C, int dtype, iseg_stream_t stream);
int iseg_bn_swish_gate_bwd_reduce(const void* dO, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                  float* partials, size_t partials_bytes, int N, int HW, int C, int dtype, iseg_stream_t stream);
int iseg_se_excite_bwd(const float* partials, int N, int HW, int C, int Cse, const float* W1, const float* W2, const float* m, const float* hpre,
                       const float* g, float* dW1, float* db1, float* dW2, float* db2, int accumulate, float* dmh, float* sums, void* ws,
                       size_t ws_bytes, iseg_stream_t stream);
int iseg_bn_swish_gate_bwd_apply(const void* dO, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                 const float* g, const float* dmh, const float* sums, float inv_n, int train, void* dx, float* dgamma,
                                 float* dbeta, int N, int HW, int C, int dtype, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Xception separable unit, activation=False (backbones/xception_common.py:14-78): relu -> DepthwiseConv2D(3, strides, dilation_rate,
 * padding="same") -> BN -> Conv2D(filters, 1), the pointwise BN left to the SyncBN kernels.  x, z [N, H, W, C] / [N, Ho, Wo, C] NHWC fp32 or
 * bf16 (dtype), w [9][C] fp32 (the Keras depthwise kernel), pointwise kernel W [Cin][Cout] fp32, statistics fp32.  With a = gamma*rstd and
 * c = beta - a*mean the BN is folded into the GEMM: v = z (diag(a) W) + c^T W; relu(x) and the BN output are never written.
 *   iseg_relu_dwconv3_stats   z = dw3x3(relu(x)); packed != NULL: iseg_bn_stats' message [sum z | sum z^2 | count] of the stored z, from
 *                             fixed-order per-tile partials in ws (iseg_relu_dwconv3_stats_workspace_bytes); packed == NULL: z only
 *   iseg_sepconv_fold         Wt [Cout][Cin] = (diag(a) W)^T and Wn [Cin][Cout] = diag(a) W in dtype (either may be NULL, not both), bias [Cout] = c^T W fp32
 *   iseg_sepconv_fold_bwd     G = z^T dV [Cin][Cout] fp32, S = colsum(dV) [Cout]: dW += diag(a) G + c S^T (dW may be NULL);
 *                             sums [2Cin] = [dbeta | dgamma], dbeta = W S, dgamma = rstd (rowsum(W o G) - mean dbeta): iseg_bn_bwd_reduce's
 *                             layout, so the SyncBN all-reduce carries it; the same launch adds this replica's own sums into dgamma / dbeta
 *                             when non-NULL (booked before that all-reduce, as _BatchNormTrainFn books them)
 *   iseg_bnfold_dwconv3_relu_bwd  D = dV Wn^T [N, Ho, Wo, C] (dtype): dz = D + alpha + beta' z staged in LDS (train: the BN backward of the
 *                             all-reduced sums with inv_n = 1 / global count; train == 0: dz = D); dx = [x > 0] dw3x3^T(dz),
 *                             dw [9][C] += sum relu(x) dz per tap (fixed-order per-tile partials in ws).
 * The two depthwise kernels stage a pixel tile plus its halo in LDS once per workgroup (relu(x) forward, dz backward) and read every tap there.
 * K = 3, stride 1 or 2 (stride 2: dilation 1), dilation <= 8, C % 8 == 0, N <= 65535, 16-byte aligned activations and w; anything else
 * returns ISEG_ERR_UNSUPPORTED.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_sepconv_supported(int N, int H, int W, int C, int stride, int dil, int dtype);
size_t iseg_relu_dwconv3_stats_workspace_bytes(int N, int H, int W, int C, int stride, int dil);
int iseg_relu_dwconv3_stats(const void* x, const float* w, void* z, float* packed, int N, int H, int W, int C, int stride, int dil, int dtype,
                            void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_sepconv_fold(const float* W, const float* mean, const float* rstd, const float* gamma, const float* beta, void* Wt, void* Wn, float* bias,
                      int Cin, int Cout, int dtype, iseg_stream_t stream);
int iseg_sepconv_fold_bwd(const float* G, const float* S, const float* W, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, float* dW, float* sums, float* dgamma, float* dbeta, int Cin, int Cout, iseg_stream_t stream);
size_t iseg_bnfold_dwconv3_relu_bwd_workspace_bytes(int N, int H, int W, int C, int stride, int dil);
int iseg_bnfold_dwconv3_relu_bwd(const void* D, const void* z, const void* x, const float* w, const float* mean, const float* rstd,
                                 const float* gamma, const float* sums, float inv_n, int train, void* dx, float* dw, int N, int H, int W, int C,
                                 int stride, int dil, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * JointPyramidUpsampling tail (layers/jpu.py:38-59, 79-88): the merged map x [N, H, W, C] feeds four branches DepthwiseConv2D(3, padding="same",
 * dilation_rate=r, use_bias=True) -> BN -> ConvNormAct(width), r = 1, 2, 4, 8.  Rate-major operands: w [4][9][C], bias [4][C],
 * z / D [4][N, H, W, C] (dtype fp32 or bf16, NHWC), mean / rstd / gamma [4][C] fp32.  The BN of every branch is folded into its pointwise GEMM
 * (iseg_sepconv_fold / iseg_sepconv_fold_bwd above), so only the depthwise side is new:
 *   iseg_jpu_dwconv3x4_stats       z_r = dw3x3_r(x) + bias_r for the four rates from ONE window of x staged in LDS (pixel tile + halo of 8);
 *                                  packed != NULL: four iseg_bn_stats messages [4][2C+1] = [sum z | sum z^2 | count] of the stored z, from
 *                                  fixed-order per-tile partials in ws; packed == NULL: z only (ws is not read)
 *   iseg_jpu_bnfold_dwconv3x4_bwd  dz_r = D_r + alpha_r + beta'_r z_r (train: the BN backward of the all-reduced sums [4][2C] = [dbeta | dgamma]
 *                                  per rate with inv_n = 1 / global count; train == 0: dz_r = D_r) staged in LDS with its halo of r;
 *                                  dx = sum_r dw3x3_r^T(dz_r) summed in registers and stored once, dw [4][9][C] += sum x dz_r per tap,
 *                                  db [4][C] += sum dz_r (fixed-order per-tile partials in ws, 10 rows per rate; train: that sum is
 *                                  identically zero over the batch of the statistics, and nothing is added).  dz is never written.
 *   iseg_jpu_partials_bytes        the bytes of ws either launcher needs (backward = 0: the statistics partials, 1: the dw / db partials); a
 *                                  null or shorter ws returns ISEG_ERR_WORKSPACE and nothing is launched
 * Stride 1, C % 8 == 0, N <= 65535, 16-byte aligned activations and vectors; anything else returns ISEG_ERR_UNSUPPORTED.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_jpu_supported(int N, int H, int W, int C, int dtype);
size_t iseg_jpu_partials_bytes(int N, int H, int W, int C, int backward);
int iseg_jpu_dwconv3x4_stats(const void* x, const float* w, const float* bias, void* z, float* packed, int N, int H, int W, int C, int dtype,
                             void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_jpu_bnfold_dwconv3x4_bwd(const void* D, const void* z, const void* x, const float* w, const float* mean, const float* rstd,
                                  const float* gamma, const float* sums, float inv_n, int train, void* dx, float* dw, float* db, int N, int H,
                                  int W, int C, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * ResNet-9 / 10 / 18 basic-block tail (backbones/resnet_blocks_small.py, BlockType2Small.call :84-119: shortcut_bn :89-90, avg_pool2d of the
 * shortcut :92-98, conv2_bn :105, add + relu :107-108):
 *   out = relu(bn2(z2) + pool_s(sc)),  sc = bn0(z0) (shortcut conv) or x (identity),  bn(v) = (v - mean) * rstd * gamma + beta
 *   pool_s = avg_pool2d(window = strides = s, "SAME"), s in {1, 2}, padded cells excluded from the divisor.
 * The shortcut input z0 / x is [N, H, W, C]; z2, out, dout, dz2 are [N, ceil(H/s), ceil(W/s), C]; NHWC fp32 or bf16 (dtype), statistics fp32.
 * Training statistics: mean / rstd from iseg_bn_stats + (all-reduce) + iseg_bn_finalize; moving statistics: moving_mean and
 * iseg_rsqrt_eps(moving_variance).  mean0 / z0 == NULL selects the identity shortcut.
 *   iseg_resblock_tail_fwd         reads z2 and the shortcut input once, writes only out (no BN output, no pooled shortcut)
 *   iseg_resblock_tail_bwd_reduce  g = dout * [out > 0]; sums [2C] = (sum g, sum g*xhat2) over the output rows, and with a BN0 shortcut
 *                                  [4C]: + (sum u, sum u*xhat0) over the full-resolution rows, u = unpool(g) / count -- each half in
 *                                  iseg_bn_bwd_reduce's layout, so the SyncBN all-reduce carries the message unchanged.  Per-workgroup
 *                                  partials go to ws (iseg_resblock_tail_workspace_bytes) and are summed in a fixed order.
 *   iseg_resblock_tail_bwd_apply   dz2 = gamma2*rstd2*(g - sums0*inv_n2 - xhat2*sums1*inv_n2), and dsc [N, H, W, C] = dz0 (the same with BN0's
 *                                  sums and inv_n0 on u) or u (identity shortcut: the caller's fork sums it with the main path's gradient).
 *                                  train == 0 (moving statistics): dz = gamma*rstd*g.  dgamma / dbeta (either BN, any may be NULL) += the
 *                                  sums by the same launch -- only while the sums are this replica's own.
 * C % 8 == 0, stride 1 or 2, 16-byte aligned tensors and vectors; anything else returns ISEG_ERR_UNSUPPORTED.  No float atomics.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_resblock_tail_supported(int C, int stride, int dtype);
size_t iseg_resblock_tail_workspace_bytes(int N, int H, int W, int C, int stride, int bn0);
int iseg_resblock_tail_fwd(const void* z2, const float* mean2, const float* rstd2, const float* gamma2, const float* beta2, const void* sc,
                           const float* mean0, const float* rstd0, const float* gamma0, const float* beta0, void* out, int N, int H, int W, int C,
                           int stride, int dtype, iseg_stream_t stream);
int iseg_resblock_tail_bwd_reduce(const void* dout, const void* out, const void* z2, const float* mean2, const float* rstd2, const void* z0,
                                  const float* mean0, const float* rstd0, float* sums, int N, int H, int W, int C, int stride, int dtype, void* ws,
                                  size_t ws_bytes, iseg_stream_t stream);
int iseg_resblock_tail_bwd_apply(const void* dout, const void* out, const void* z2, const float* mean2, const float* rstd2, const float* gamma2,
                                 const void* z0, const float* mean0, const float* rstd0, const float* gamma0, const float* sums, float inv_n2,
                                 float inv_n0, int train, void* dz2, void* dsc, float* dgamma2, float* dbeta2, float* dgamma0, float* dbeta0,
                                 int N, int H, int W, int C, int stride, int dtype, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Exchange step of the data-parallel path: distribution/distribution_utils.py:158-169 all_reduce_values -> ReplicaContext.all_reduce(SUM)
 * (SyncBN statistics layers/keras3/bn.py:60-117, gradient sums), over RCCL on xGMI.  One process per GPU: rank 0 creates the 128-byte id
 * and hands it to the other ranks through the host program; every rank then calls iseg_comm_init.  iseg_allreduce_sum works in place and is
 * stream-ordered.  RCCL is resolved at run time (no link dependency); ISEG_ERR_UNSUPPORTED when it cannot be found.
 * (The Python host of this repository keeps using torch.distributed, which drives the same RCCL -- iseg_amd/dist.py.)
 * --------------------------------------------------------------------------------------------------------- */
typedef void* iseg_comm_t;
int iseg_comm_unique_id(void* id128);
int iseg_comm_init(iseg_comm_t* comm, int world_size, int rank, const void* id128);
int iseg_allreduce_sum(iseg_comm_t comm, void* buf, size_t count, int dtype, iseg_stream_t stream);
int iseg_comm_destroy(iseg_comm_t comm);

/* ---------------------------------------------------------------------------------------------------------
 * Layout / elementwise
 * --------------------------------------------------------------------------------------------------------- */
/* Deferred parameter-gradient reductions.  Keras accumulates nothing across ops -- this is a scheduling service of the library: between
 * begin and end, every two-stage reduction of an entry point (iseg_layernorm_bwd, iseg_dwconv2d_bwd_weight, iseg_colsum) whose output lies
 * inside [grad_base, grad_base + grad_bytes) and accumulates into it keeps its partial sums in `arena` (>= 1 MiB, caller-owned) instead of the
 * call's workspace and is queued; iseg_deferred_flush runs one launch over the queue (same fixed summation order as the immediate reduce).
 * The caller flushes before anything reads the gradient buffer (optimizer, clipping, all-reduce).  Single stream, not re-entrant. */
int iseg_deferred_begin(void* grad_base, size_t grad_bytes, void* arena, size_t arena_bytes, iseg_stream_t stream);
int iseg_deferred_flush(iseg_stream_t stream);
int iseg_deferred_end(iseg_stream_t stream);
int iseg_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, iseg_stream_t stream);
/* K-contiguous copies of the bf16 compute kernels for the forward GEMMs (keras Dense / 1x1 Conv2D kernels are [K][N]; with both operands
 * K-contiguous the LDS-DMA GEMM serves the forward pass too).  `count` bf16 matrices inside `src`, transposed into `dst`;
 * table (device, int64 [count][4]) = {src element offset, dst element offset, rows, cols}; max_tiles = max over matrices of
 * ceil(rows/64) * ceil(cols/64).  One launch per optimizer step (iseg_amd/nn.py wt()). */
int iseg_transpose_batched(const void* src, void* dst, const int64_t* table, int count, int max_tiles, iseg_stream_t stream);
/* dst[k][n] = src[k][n]*colscale[n]: layer-scale folded Dense kernel for the dgrad of backbones/convnext.py:54-57 */
int iseg_scale_cols_cast(const float* src, const float* colscale, void* dst, int64_t rows, int cols, int dst_dtype,
                         iseg_stream_t stream);
/* patches of keras.layers.Conv2D(padding="same"/"valid", strides, dilation_rate): col[m][(i*KW+j)*C+c], row stride ldc */
int iseg_im2col(const void* x, int in_dtype, void* col, int out_dtype, int N, int H, int W, int C, int KH, int KW, int sh, int sw,
                int dh, int dw, int pt, int pl, int Ho, int Wo, int64_t ldc, iseg_stream_t stream);
int iseg_col2im(const void* dcol, void* dx, int N, int H, int W, int C, int KH, int KW, int sh, int sw, int dh, int dw, int pt,
                int pl, int Ho, int Wo, int64_t ldc, int dtype, iseg_stream_t stream);
/* out[b][c] (+)= scale * sum_r x[b][r][c]: bias gradients; tf.reduce_mean over H,W (layers/model_builder.py:266) */
size_t iseg_colsum_workspace_bytes(int batch, int64_t rows, int C);
int iseg_colsum(const void* x, int64_t ldx, int64_t batch_stride, int batch, int64_t rows, int C, float* out, float scale,
                int accumulate, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* y[b][r][:] (+)= scale*v[b][:]: ImageLevelBlock broadcast (layers/model_builder.py:268) and the pooling gradient */
int iseg_broadcast_rows(const void* v, int v_dtype, void* y, int64_t ldy, int64_t batch_stride, int batch, int64_t rows, int C,
                        float scale, int accumulate, int dtype, iseg_stream_t stream);
int iseg_axpby(const void* a, const void* b, void* y, float alpha, float beta, int64_t n, int dtype, iseg_stream_t stream);
/* dst0[i] += src[i], dst1[i] += src[n+i] (NULL destinations are skipped): dbeta | dgamma of a normalisation layer's packed backward sums */
int iseg_accumulate_pair(const float* src, int n, float* dst0, float* dst1, iseg_stream_t stream);
/* y = x * s_dev[0] (chain rule with a device-resident scalar; no host read) */
int iseg_scale_dev(const void* x, const float* s_dev, void* y, int64_t n, int dtype, iseg_stream_t stream);
int iseg_rowscale(const void* x, const float* s, void* y, int64_t rows, int C, int64_t rows_per_group, int dtype,
                  iseg_stream_t stream);
/* keras.layers.Dropout: y = x*mask/(1-rate); mask = f(seed, index) so backward = same call on dy.
 * seed_offset (device pointer, may be NULL) is added to `seed` by the kernel: a training step replayed from a HIP graph has frozen launch
 * arguments, so its draw counter lives in device memory (iseg_amd/graphs.py); same meaning in the two drop-path entry points. */
int iseg_dropout(const void* x, void* y, int64_t n, float rate, uint64_t seed, const uint64_t* seed_offset, int dtype, iseg_stream_t stream);
/* utils/drops.py:14-20: s[n] = floor(keep + u_n)/keep */
int iseg_drop_path_mask(float* s, int n, float keep_prob, uint64_t seed, const uint64_t* seed_offset, iseg_stream_t stream);
/* P masks of n samples each in one launch (s [P, n], keep_probs [P] on the device): the drop_path call sites of one training step */
int iseg_drop_path_masks(float* s, const float* keep_probs, int P, int n, uint64_t seed, const uint64_t* seed_offset, iseg_stream_t stream);
int iseg_fill_f32(float* p, float value, int64_t n, iseg_stream_t stream);
/* DCNv2's sampling half (layers/dcn_v2.py:114-229; FaPN's FeatureAlignment, layers/fapn.py:44-80): offset [N,H,W,27] = the offset convolution's output
 * (9 x (dy, dx), then 9 mask logits); col [N,H,W,9,C] = sigmoid(logit_p) * bilinear sample of x (zero-padded by 1) at (h + ky + dy_p, w + kx + dx_p), with the
 * reference's clipping of the position and both corners to [0, H+1] x [0, W+1] and weights from the clipped values.  The layer's output is then the GEMM
 * col [N H W, 9 C] x kernel [9 C, filters] (:230-240).  bwd: dx fp32 (64-bit fixed-point accumulation: deterministic), doffset [N,H,W,27] in storage type. */
int iseg_dcnv2_sample_fwd(const void* x, const void* offset, void* col, int N, int H, int W, int C, int dtype, iseg_stream_t stream);
size_t iseg_dcnv2_sample_bwd_workspace_bytes(int N, int H, int W, int C);
int iseg_dcnv2_sample_bwd(const void* x, const void* offset, const void* dcol, float* dx_f32, void* doffset, int N, int H, int W, int C, int dtype,
                          void* ws, size_t ws_bytes, iseg_stream_t stream);
/* EVA-02 (backbones/eva/*).
 * iseg_qkv_rope: packed attention rows qkv [rows = B * tokens][3 C] = [q | k | v] -> out (out == qkv: in place): q += q_bias, v += v_bias (the fused projection's
 *   bias [q_bias | 0 | v_bias], attention.py:100-112; either may be NULL), then the rotary embedding on q and k of the tokens t >= prefix
 *   (apply_rot_embed_cat, rotar_embedding_cat.py:117-135; the class token keeps its values, attention.py:136-146).  emb fp32 [tokens - prefix][2 head_dim]
 *   = [sin | cos] (RotaryEmbeddingCat.get_embed), NULL = no rotation.  inverse = 1 applies the transposed rotation (the backward pass; pass NULL biases).
 * iseg_glu_fwd / _bwd: out = act(gate) * x on strided [rows, cols] operands (SwiGLU: two Dense outputs, swiglu.py:88-92; GluMlp: the two column halves
 *   of one Dense output, glumlp.py:96-103); act = ISEG_ACT_GELU | ISEG_ACT_SWISH | ISEG_ACT_SIGMOID; bwd: dgate = dout x act'(gate), dx = dout act(gate).
 *   Operands with cols / row strides that are multiples of 8 and 16-byte aligned bases move 16-byte pieces; anything else (EVA02-large: 2730 columns) takes
 *   the one-element-per-lane form. */
int iseg_qkv_rope(const void* qkv, void* out, const float* q_bias, const float* v_bias, const float* emb, int64_t rows, int tokens, int prefix, int C, int head_dim,
                  int inverse, int dtype, iseg_stream_t stream);
int iseg_glu_fwd(const void* gate, int64_t ld_gate, const void* x, int64_t ld_x, void* out, int64_t ld_out, int64_t rows, int cols, int act, int dtype,
                 iseg_stream_t stream);
int iseg_glu_bwd(const void* dout, int64_t ld_dout, const void* gate, int64_t ld_gate, const void* x, int64_t ld_x, void* dgate, int64_t ld_dgate,
                 void* dx, int64_t ld_dx, int64_t rows, int cols, int act, int dtype, iseg_stream_t stream);
/* keras.activations.relu / gelu / sigmoid / swish where no GEMM epilogue is available; bwd: dx = dy*act'(aux), aux = pre-activation */
int iseg_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, iseg_stream_t stream);
int iseg_act_bwd(const void* dy, const void* aux, void* dx, int64_t n, int act, int dtype, iseg_stream_t stream);
/* tf.concat(axis=-1) as slice writes: dst[r][0:cols] = src[r][0:cols] (layers/aspp.py:69) */
int iseg_copy2d(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int cols, int dtype,
                iseg_stream_t stream);
/* sliding-window inference accumulator (core_inference.py:254-301): dst[r][c] += src[r][c]; y[r][:] = x[r][:]*s[r] */
int iseg_add2d_f32(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t rows, int64_t cols, iseg_stream_t stream);
int iseg_scale_rows_f32(const float* x, const float* s, float* y, int64_t rows, int C, iseg_stream_t stream);
/* ConvNeXt layer-scale parameter gradients from Z = g^T dout (see iseg_amd/blocks.py) */
size_t iseg_layerscale_grads_workspace_bytes(int K, int N);
int iseg_layerscale_grads(const float* Z, const float* W2, const float* b2, const float* gamma, const float* S, float* dW2,
                          float* dgamma, float* db2, int K, int N, int accumulate, void* ws, size_t ws_bytes,
                          iseg_stream_t stream);
/* The same from the UNREDUCED split-K slabs of the product Z = g^T dout (iseg_gemm with defer_reduce on an orientation that carries the
 * ones-row: slabs [nslabs][K + 1][N] fp32, row K = column sums of dout): Z and S are formed in slab order while they are read, so the slab-sum
 * launch and the Z tensor disappear.  N % 4 == 0. */
int iseg_layerscale_grads_slabs(const float* slabs, int nslabs, const float* W2, const float* b2, const float* gamma, float* dW2, float* dgamma,
                                float* db2, int K, int N, int accumulate, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* The same plus, in the SAME launch, the slab sum of the pair launch's other product (iseg_gemm_tn_pair: dW1 = y2^T dH with its ones-row db1,
 * backbones/convnext.py:51-57 backward): out0[j] (+)= sum_p partials2[p * n2 + j] for j < n0, out1[j - n0] likewise beyond (out1 may be null) --
 * what iseg_gemm_reduce would have launched (same slab order, same arithmetic).  partials2 must not alias ws; n2, n0 % 4 == 0, 16-byte aligned. */
int iseg_layerscale_grads_slabs_reduce(const float* slabs, int nslabs, const float* W2, const float* b2, const float* gamma, float* dW2,
                                       float* dgamma, float* db2, int K, int N, int accumulate, void* ws, size_t ws_bytes,
                                       const float* partials2, int P2, int64_t n2, float* out0, float* out1, int64_t n0, int accumulate2,
                                       iseg_stream_t stream);
/* ---------------------------------------------------------------------------------------------------------
 * tf.image.resize (half-pixel, no antialias): utils/common.py:107-134 resize_image
 * --------------------------------------------------------------------------------------------------------- */
int iseg_resize_bilinear_fwd(const void* x, int in_dtype, void* y, int out_dtype, int N, int Hi, int Wi, int Ho, int Wo, int C,
                             iseg_stream_t stream);
size_t iseg_resize_bilinear_bwd_workspace_bytes(int N, int Hi, int Wi, int Ho, int Wo, int C);
int iseg_resize_bilinear_bwd(const void* dy, int dy_dtype, void* dx, int dx_dtype, const void* dx_add, int N, int Hi, int Wi,
                             int Ho, int Wo, int C, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* tf.compat.v1.image.resize(x, size, method="bilinear", align_corners=True) (backbones/hrnet.py:303-304, 523-524): source coordinate
 * dst*(in-1)/(out-1), same lerp order; the backward uses iseg_resize_bilinear_bwd_workspace_bytes */
int iseg_resize_bilinear_ac_fwd(const void* x, int in_dtype, void* y, int out_dtype, int N, int Hi, int Wi, int Ho, int Wo, int C,
                                iseg_stream_t stream);
int iseg_resize_bilinear_ac_bwd(const void* dy, int dy_dtype, void* dx, int dx_dtype, const void* dx_add, int N, int Hi, int Wi, int Ho, int Wo,
                                int C, void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_resize_nearest_i32(const int32_t* x, int32_t* y, int N, int Hi, int Wi, int Ho, int Wo, int C, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * losses/catecrossentropy_ignore_label.py:44-88 weighted_loss (CategoricalCrossentropy(from_logits), NONE) and
 * metrics/seg_metric_wrapper.py:89-102 + metrics/confusion_matrix.py:65-143.
 * logits [P,C] fp32, labels [P] int32.  loss_px [P] (optional), loss_sum[0] = loss_sum_scale * sum_p loss_p,
 * dlogits = grad_scale * grad_px[p] * w_p * (softmax - onehot) (optional; grad_px NULL = 1).
 * --------------------------------------------------------------------------------------------------------- */
size_t iseg_softmax_ce_workspace_bytes(int64_t P, int C);
int iseg_softmax_ce_ignore(const float* logits, const int32_t* labels, const float* class_w, int64_t P, int C, int ignore_label,
                           float* loss_px, float* loss_sum, float loss_sum_scale, float* dlogits, float grad_scale,
                           const float* grad_px, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* iseg_softmax_ce_ignore that also performs iseg_argmax_confusion on the same logits / labels (cm[y*C + argmax] += 1 for kept,
 * in-range labels; first maximal index): the training step's loss and running-mIoU update in ONE pass over the logits */
int iseg_softmax_ce_confusion(const float* logits, const int32_t* labels, const float* class_w, int64_t P, int C, int ignore_label,
                              float* loss_px, float* loss_sum, float loss_sum_scale, float* dlogits, float grad_scale,
                              const float* grad_px, uint64_t* cm, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* focal variant (use_focal_loss of losses/catecrossentropy_ignore_label.py:27-37 = keras CategoricalFocalCrossentropy, from_logits):
 * p = clip(softmax(logits)[y], 1e-7, 1 - 1e-7);  loss = w * alpha * (1 - p)^gamma * (-log p);  same outputs and masking rules */
int iseg_softmax_focal_ce_ignore(const float* logits, const int32_t* labels, const float* class_w, int64_t P, int C, int ignore_label,
                                 float alpha, float gamma, float* loss_px, float* loss_sum, float loss_sum_scale, float* dlogits,
                                 float grad_scale, const float* grad_px, void* ws, size_t ws_bytes, iseg_stream_t stream);
/* pred_out [P] int32 (optional) = first argmax; cm [C*C] uint64 counts += (label != ignore) at [label][pred] */
int iseg_argmax_confusion(const float* logits, const int32_t* labels, int64_t P, int C, int ignore_label, int32_t* pred_out,
                          unsigned long long* cm, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * metrics/confusion_matrix.py:65-143 confusion_matrix and :146-231 batch_confusion_matrix (tf.scatter_nd of the weights at
 * [b, label, prediction]), the arithmetic under metrics/mean_iou.py:16-55 get_class_confusion_matrix / get_batch_class_confusion_matrix
 * and :112-130 MeanIOU.update_state(y_true, y_pred, sample_weight), from label and prediction MAPS (iseg_argmax_confusion takes logits).
 *   labels, preds [batch, n] int32;  weights [batch, n]: NULL (ISEG_CM_W_NONE), one byte per element (ISEG_CM_W_U8: uint8 / bool) or fp32
 *   cm [batch, C, C] int64, row = label, column = prediction; accumulate = 0 clears it first (stream-ordered), 1 adds to it
 *   counters [8] uint64, ADDED to (the caller clears them)
 * Per element (b, i), in this order:
 *   - use_ignore and label == ignore_label: skipped, nothing else about it is examined;
 *   - each of these that holds bumps its counter, and the element then contributes nothing (the reference's assertions :115-132, which
 *     raise; this entry point counts and goes on):  counters[0] label < 0;  [1] prediction < 0;  [2] label >= C;  [3] prediction >= C;
 *     [4] (F32) the weight is not finite or |w * 2^w_exp| >= 2^39;
 *   - counters[5] (F32) w * 2^w_exp is no integer: an element that passed the checks above is still counted, rounded to nearest even;
 *   - counters[6..7] are not touched;
 *   - cm[b][label][pred] += 1 (NONE), the byte's value 0..255 (U8), or llrint((double)w * 2^w_exp) (F32).
 * Integer arithmetic only: the scale is a power of two (exact), the bins are 64-bit, integer sums do not depend on their order.  Two runs,
 * or any permutation of an image's elements, give the same bits; no floating-point atomic is used.  The caller picks w_exp = 38 - ex with
 * max |w| = m * 2^ex, m in [0.5, 1) (frexp; 0 when every weight is 0): max |w| * 2^w_exp lies in [2^37, 2^38), and with n <= 2^24 elements
 * per image no bin reaches 2^62.  The value in fixed point differs from the real sum of a bin's k weights by at most k * 2^-(w_exp + 1),
 * i.e. k * max|w| * 2^-38.  iseg_confusion_absmax_f32 gives max |w|: max_bits[0] = the largest bit pattern of |w_i| (for non-negative
 * floats the integer order is the float order, so the integer atomic maximum is exact); a NaN or Inf shows as a pattern >= 0x7f800000.
 * Limits: 1 <= C <= 256 in every mode; |w_exp| <= 1000; F32: n <= ISEG_CM_F32_MAX_N, else ISEG_STATUS_UNSUPPORTED before any memory is touched;
 * NONE / U8: a workgroup counts the elements it sees of one image in 32-bit bins, so with gx = min(ceil(n / ISEG_CM_SLICE),
 * max(1, cap / min(batch, cap))) workgroups per image, ceil(ceil(n / ISEG_CM_SLICE) / gx) * ISEG_CM_SLICE must not exceed
 * 16 843 009 = floor((2^32 - 1) / 255).  cap is the number of workgroups the 256 CUs hold at once with the histogram's LDS, at most four per CU:
 * ISEG_CM_GRID_CAP up to C = 101 (C = 71 with fp32 weights), 256 from C = 144 (102) on.  So every n <= 16 842 752 passes at any batch and any C (2^24 + 5 included), and
 * n <= 2^32 at batch 1; beyond, ISEG_STATUS_UNSUPPORTED.  Argument errors (ISEG_STATUS_ARG, nothing launched): a null labels / preds / cm / counters, batch <= 0, n <= 0,
 * C outside 1..256, an unknown wmode, weights == NULL with wmode != 0.  No workspace: cm and counters are all the launcher needs.
 * iseg_confusion_supported is pure host: 1 <= C <= 256 and wmode in {0, 1, 2}.
 * --------------------------------------------------------------------------------------------------------- */
#define ISEG_CM_W_NONE 0   /* every element counts 1 */
#define ISEG_CM_W_U8   1   /* weights: one byte per element, its value (0..255) is added */
#define ISEG_CM_W_F32  2   /* weights: fp32, accumulated as fixed point (above) */
#define ISEG_CM_SLICE 4096          /* elements of one image a workgroup consumes per trip of its loop */
#define ISEG_CM_GRID_CAP 1024       /* workgroups per launch, at most (fewer where a CU holds fewer than four histograms) */
#define ISEG_CM_F32_MAX_N 16777216  /* 2^24 */
int iseg_confusion_supported(int C, int wmode);
int iseg_confusion_absmax_f32(const float* w, int64_t n, uint32_t* max_bits, iseg_stream_t stream);
int iseg_confusion_batched(const int32_t* labels, const int32_t* preds, const void* weights, int wmode, int w_exp, int64_t batch, int64_t n,
                           int C, int use_ignore, int ignore_label, long long* cm, int accumulate, unsigned long long* counters,
                           iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * losses/ohem.py:11-39 ohem_selector -- online hard example mining on the per-position loss vector, restated literally (the file carries a
 * "WIP" comment, yet core_model.py:480-514 hands get_ohem_fn(thresh) to the main output's cross-entropy as post_compute_fn).
 *
 * iseg_ohem_label_prob: prob [P] = max_c softmax(logits_p)_c * onehot_pc (:18-20) = the labelled class's probability, exactly 0 on a zero row.
 *   The label-to-row rule is the one of iseg_softmax_ce_ignore (ignore_label == 0 shifts the labels down by one; a class outside [0, C) is
 *   the zero row), so prob and loss agree on the zero rows.  fp32, max-subtracted, one pass, rows staged through LDS as in the loss kernel.
 *
 * iseg_ohem_select: values [P], loss [P] (may be values), min_kept_total = min_kept * batch_size.
 *   values_are_loss = 0 (thresh given, values = prob, :17-33):  nnz = #{values != 0};  k = min(min_kept_total, nnz - 1);
 *        min_threshold = sort(values, DESCENDING)[k], or 0 when nnz == 0;  threshold = max(min_threshold, thresh);  keep = values < threshold
 *   values_are_loss = 1 (thresh None, values = loss, :34-37):   threshold = sort(values, DESCENDING)[min_kept_total];  keep = values > threshold
 *   keep [P]            1.0f / 0.0f, both compares strict: the grad_px of iseg_softmax_ce_ignore (the threshold is not differentiated)
 *   loss_out [P]        (optional, may be loss) keep ? loss : 0
 *   masked_sum [1]      (optional) sum_scale * sum_p loss_out_p, two stages in a fixed order
 *   threshold_out [1], nnz_out [1]   the threshold compared against and the count of non-zero values
 *   state [ISEG_OHEM_STATE_INTS] int32 and partials [ISEG_OHEM_PARTIAL_FLOATS] fp32 (needed with masked_sum) are scratch of fixed,
 *   shape-independent size, zeroed by the call on its stream, undefined on return.  There is no opaque workspace and no workspace function.
 * The k-th largest value comes from a most-significant-digit radix select instead of the reference's full sort: four 8-bit passes over the
 * order-preserving unsigned image of the float bits (any finite value, either sign), per-workgroup LDS histograms flushed with integer
 * atomics, a one-workgroup launch between passes that picks the digit and carries the remaining rank, which lives on the device.  Every
 * dependency between workgroups is a launch boundary; no floating-point atomics; no host read, no host-to-device copy, no allocation: the
 * call captures into a graph and is bit-reproducible.  Non-finite values are binned like any other bit pattern.  Errors: a null required
 * pointer, P outside 1..2^31-1 (int32 counters), C outside 1..256, keep aliasing values / loss / loss_out, min_kept_total < 0, and with
 * values_are_loss an index min_kept_total >= P.
 * --------------------------------------------------------------------------------------------------------- */
#define ISEG_OHEM_STATE_INTS 1032
#define ISEG_OHEM_PARTIAL_FLOATS 1024
int iseg_ohem_label_prob(const float* logits, const int32_t* labels, int64_t P, int C, int ignore_label, float* prob, iseg_stream_t stream);
int iseg_ohem_select(const float* values, const float* loss, int64_t P, int64_t min_kept_total, float thresh, int values_are_loss, float* keep,
                     float* loss_out, float* masked_sum, float sum_scale, float* threshold_out, int32_t* nnz_out, int32_t* state,
                     float* partials, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * losses/mask_loss.py:10-201 MaskLoss (+ dice(), :159-200) on losses/seg_loss_base.py:12-95 SegLossBase: per-class sigmoid (focal) loss,
 * per-image dice loss and softmax cross-entropy, the ignore label carried as a Keras loss mask (a mean over VALID pixels).
 * logits [B, HW, C] fp32, labels [B, HW] int32 (already at the logits' size), C <= 256.  flags = ISEG_MASKLOSS_* ; at least one term.
 *   loss_px [B*HW]  (optional) the masked per-pixel loss, dice value of the image included      (reduction = none)
 *   loss_mean[0]    (optional) loss_scale * sum(valid * loss) / (sum(valid) + 1e-7)             (sum_over_batch_size under the mask)
 *   dlogits         (optional) grad_scale * d(mean)/d(logits); with grad_px [B*HW] instead grad_scale * sum_p grad_px[p] d(loss_px[p])/d(logits)
 * Two streaming passes over the logits and one fixed-order finalize launch in between; no floating-point atomics, no host read.
 * --------------------------------------------------------------------------------------------------------- */
#define ISEG_MASKLOSS_SIGMOID 1
#define ISEG_MASKLOSS_DICE 2
#define ISEG_MASKLOSS_CE 4
#define ISEG_MASKLOSS_FOCAL_SIGMOID 8
#define ISEG_MASKLOSS_FOCAL_CE 16
#define ISEG_MASKLOSS_CLASS_BALANCING 32
size_t iseg_mask_loss_workspace_bytes(int B, int64_t HW, int C);
int iseg_mask_loss(const float* logits, const int32_t* labels, int B, int64_t HW, int C, int ignore_label, int flags, float sigmoid_coef,
                   float dice_coef, float ce_coef, float* loss_px, float* loss_mean, float loss_scale, float* dlogits, float grad_scale,
                   const float* grad_px, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * metrics/sod/sod_metrics.py on metrics/sod/sod_metric_utils.py:17-109: TFMAEMetric (:114-190), TFSmeasureMetric (:193-438),
 * TFEmeasureMetric (:441-743), TFFmeasureMetric (:746-938) and, with ISEG_SOD_WFM, TFWeightedFmeasureMetric (:941-1076, the SciPy
 * distance transform and convolution of :35-111 included).  B images per call, each scored on its own.
 *   pred [B,H,W]   fp32 in [0,1] (pred_is_u8 = normalize = 0), or uint8 with normalize = 1 (prepare_data, sod_metric_utils.py:67-95)
 *   gt   [B,H,W]   one byte per pixel: non-zero is foreground, > 128 under normalize
 *   state [ISEG_SOD_STATE_DOUBLES] += the per-image record summed in image order, count[0] += B   (both optional, together):
 *       0 MAE, 1 S-measure, 2 adaptive E, 3 adaptive F, 4 weighted F, 5.. E curve [256], 261.. F curve [257], 518.. precision [257],
 *       775.. recall [257]; curve index i is threshold 255 - i (E) or 256 - i (precision / recall / F), as the reference orders them
 *   per_image_out [B, ISEG_SOD_STATE_DOUBLES]  (optional) the same record of every image
 *   ints_out [B, ISEG_SOD_INTS] (optional): 0.. foreground histogram [256] of int(p * 255.0f), 256.. background histogram [256],
 *       512 foreground count, 513 count of p >= thr, 514 of p >= thr && g, 515 cy, 516 cx (centroid + 1), 517 bits of the fp32 adaptive threshold
 *   dist2_out / nearest_out [B,H,W] int32 (optional, ISEG_SOD_WFM): exact squared Euclidean distance to the nearest foreground pixel and its
 *       row-major index (the smallest index among equidistant ones); unwritten for an image without foreground
 * Two streaming passes over pred and gt with a mid step between them, the weighted F-measure's own kernels, a per-image finalize and one
 * launch that adds to the state.  Float sums are fixed-order fp64 partials, integers use integer atomics; no host read.
 * --------------------------------------------------------------------------------------------------------- */
#define ISEG_SOD_WFM 1
#define ISEG_SOD_STATE_DOUBLES 1032
#define ISEG_SOD_INTS 544
size_t iseg_sod_metrics_workspace_bytes(int B, int H, int W, int flags);
int iseg_sod_metrics(const void* pred, int pred_is_u8, const uint8_t* gt, int normalize, int B, int H, int W, int flags, double alpha,
                     double beta_fm, double beta_wfm, double* state, long long* count, int32_t* ints_out, double* per_image_out,
                     int32_t* dist2_out, int32_t* nearest_out, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * metrics/sod/fmeasurev2.py: TFBaseHandler.update_state (:117-237: _get_statistics :156-177, _adaptively_binarizing :179-195,
 * _dynamically_binarizing :197-237) and the compute_metric of its ten handlers: TFIOUHandler (:336-340), TFSpecificityHandler (:378-382),
 * TFDICEHandler (:424-428), TFOverallAccuracyHandler (:466-470), TFKappaHandler (:509-523), TFPrecisionHandler (:561-565),
 * TFRecallHandler (:603-607), TFFPRHandler (:650-654), TFBERHandler (:692-700), TFFmeasureHandler (:741-749).  B images per call, each
 * scored on its own, n_handlers handlers (1..ISEG_SODV2_MAX_HANDLERS) from ONE pass over the pixels.
 *   pred [B,H,W]   fp32 in [0,1] (pred_is_u8 = normalize = 0), or uint8 with normalize = 1 (prepare_data, sod_metric_utils.py:67-95)
 *   gt   [B,H,W]   one byte per pixel: non-zero is foreground, > 128 under normalize
 *   kinds_h / modes_h / betas_h [n_handlers]  HOST arrays, read during the call and passed on by value: ISEG_SODV2_<kind>, an OR of
 *       ISEG_SODV2_DYNAMIC / ADAPTIVE / BINARY (0 is allowed: the handler records nothing), and beta of the F-measure (read for that kind only)
 *   state [n_handlers, ISEG_SODV2_HANDLER_DOUBLES] += the per-image records summed in image order, count[0] += B  (both optional, together).
 *       A handler's record: 0..255 the dynamic curve, index i is threshold 255 - i (TP = pixels of the foreground in bins >= 255 - i of
 *       int(p * 255.0f), the fp32 product); 256 the score at the adaptive threshold p >= float(min(2 mean p, 1)); 257 the score at p > 0.5;
 *       258..261 tp, fp, tn, fn at p > 0.5 (the dataset-based binary mode sums them); 262..263 zero.  Slots of a mode the handler did not
 *       ask for are 0.
 *   per_image_out [B, n_handlers, ISEG_SODV2_HANDLER_DOUBLES]  (optional) the same record of every image
 *   ints_out [B, ISEG_SODV2_INTS] (optional): 0.. foreground histogram [256] of int(p * 255.0f), 256.. background histogram [256],
 *       512 foreground count, 513 count of p >= thr, 514 of p >= thr && g, 515 count of p > 0.5, 516 of p > 0.5 && g, 517 bits of the fp32
 *       adaptive threshold, 518..519 zero.  For an fp32 prediction 513, 514 and 517 are 0 unless some handler has ISEG_SODV2_ADAPTIVE.
 * FN = FG - TP and TN = BG - FP with FG = count_nonzero(gt) (:129-130, :175-176).  Scores are fp64 on the exact counts; safe_divide tests the
 * integer denominator, and Kappa's 1 - p_e == 0 is (tp+fp)(tp+fn) + (tn+fn)(tn+tp) == total^2 in int64.  That second product is the
 * reference's own formula (:519), kept as it writes it.
 * uint8: one streaming pass (the 2 x 256 histogram of raw grey levels by gt) and one wavefront per image that derives every other quantity from
 * those 512 integers.  fp32: one streaming pass; a threshold step and a second pass only if some handler has ISEG_SODV2_ADAPTIVE.  Then a
 * per-image finalize and one launch that adds to the state.  Integer atomics and fixed-order fp64 partials only; no host read, no
 * host-to-device copy: the call captures into a graph.  Errors: n_handlers outside 1..32, an unknown kind or mode bit, H or W > 16384.
 * --------------------------------------------------------------------------------------------------------- */
#define ISEG_SODV2_IOU 0
#define ISEG_SODV2_SPECIFICITY 1
#define ISEG_SODV2_DICE 2
#define ISEG_SODV2_OA 3
#define ISEG_SODV2_KAPPA 4
#define ISEG_SODV2_PRECISION 5
#define ISEG_SODV2_RECALL 6
#define ISEG_SODV2_FPR 7
#define ISEG_SODV2_BER 8
#define ISEG_SODV2_FMEASURE 9
#define ISEG_SODV2_DYNAMIC 1
#define ISEG_SODV2_ADAPTIVE 2
#define ISEG_SODV2_BINARY 4
#define ISEG_SODV2_MAX_HANDLERS 32
#define ISEG_SODV2_HANDLER_DOUBLES 264
#define ISEG_SODV2_INTS 520
size_t iseg_sod_fmv2_workspace_bytes(int B, int H, int W, int n_handlers);
int iseg_sod_fmv2(const void* pred, int pred_is_u8, const uint8_t* gt, int normalize, int B, int H, int W, int n_handlers,
                  const int32_t* kinds_h, const int32_t* modes_h, const double* betas_h, double* state, long long* count, int32_t* ints_out,
                  double* per_image_out, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * ops/ccl.py: label_components (:28-36) -- connected-components labelling, N images per call, each on its own (tf.map_fn over the batch, :30-34).
 *   mask   [N,H,W]  int32 (mask_is_u8 = 0) or one byte per pixel (mask_is_u8 = 1: uint8 / bool).  ANY non-zero value is foreground.  The
 *                   reference takes int32 in {0,1} only and hands every other value back negated (-binary_img is compared with -1 alone,
 *                   :52, :80), which is no labelling and is not reproduced.
 *   labels [N,H,W]  0 on the background; on the foreground the number of the pixel's 4-connected component: neighbours up, left, right, down
 *                   (NEIGHBORS_COORDS :11-16), a neighbour outside the image does not count (:188-201), so rows do not wrap and images never
 *                   share a component.  Components are numbered 1, 2, 3, ... in the raster order of their first pixel (find_components :75-92:
 *                   the loop over i = row * width + col, label += 1 at every pixel still unlabelled, then the flood fill search :117-160).
 *                   The reduce_sum <= 1 shortcut (:48-54) returns the input, which is the labelling of such an image: no special case.
 *   counts [N]      components per image = the largest label of the image (0 for an empty one)
 *   row_base [N,H]  scratch, undefined on return
 * labels doubles as the parent array of a union-find that links the larger root under the smaller one, so a component's root is its first
 * raster pixel and its number is 1 + the count of roots with a smaller index; mask and labels therefore cannot be the same buffer.  There is
 * no opaque workspace and no workspace function: all memory is these three typed, shape-sized buffers.  Six launches (tile-local union-find in
 * LDS, tile seams, flatten + root count per row, per-image scan, in-row rank, finalise), integer atomics only, no floating point, exact
 * grids, no wait on another workgroup; no host read, no host-to-device copy, no allocation: the call captures into a graph.  The result is
 * a function of the mask alone (bit-reproducible).  Errors: a null pointer, N outside 1..65535, H or W outside 1..16384 (H * W + 1 has to
 * fit an int32), mask == labels.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_ccl_label(const void* mask, int mask_is_u8, int N, int H, int W, int32_t* labels, int32_t* counts, int32_t* row_base,
                   iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * optimizers/modern/adamw.py:13-74, optimizers/modern/sgd.py:12-51 over the flat parameter buffer.
 * Every tensor is padded to a multiple of 256 elements; seg_of_block[b] = tensor index of 256-element block b
 * (-1 = padding).  hp (device): [lr, sqrt(1-b2^t)/(1-b1^t), grad_scale, clipvalue(<=0 off)].
 *   AdamW_EXT: g <- NaN->0 (adamw.py:63-74) -> clip -> decoupled decay -> m, v (, v_hat = max(v_hat, v) when vhat != NULL: amsgrad,
 *              adamw.py:54-57) -> w.       SGD_EXT: no NaN scrub; nesterov as sgd.py:46-49.
 *   Clipping = Keras' base optimizer (_clip_gradients), which the reference drives through get_optimizer(clipnorm, clipvalue)
 *   (core_optimizer.py:170-183): clipnorm is PER VARIABLE (tf.clip_by_norm), global_clipnorm over all variables
 *   (tf.clip_by_global_norm), clipvalue per element; at most one of them is active.  The squared norms come from iseg_grad_sqnorm
 *   (fixed-order sums: 256-element blocks -> variables -> total; seg_first_block [nseg + 1] = first block of each variable;
 *   block_ws [nblocks] floats of scratch; seg_l2 / w as in the SGD step or NULL).
 * --------------------------------------------------------------------------------------------------------- */
int iseg_grad_sqnorm(const float* g, const float* w, const int32_t* seg_of_block, const int32_t* seg_first_block, const float* seg_l2,
                     const float* hp, int scrub_nan_grads, float* block_ws, float* seg_sq, float* global_sq, int64_t nblocks, int nseg,
                     iseg_stream_t stream);
int iseg_adamw_step(float* w, const float* g, float* m, float* v, float* vhat, void* w_bf16, const int32_t* seg_of_block,
                    const float* seg_lr_mult, const float* seg_wd, const float* hp, float beta1, float beta2, float eps,
                    const float* seg_sq, float clipnorm, const float* global_sq, float global_clipnorm, int64_t nblocks,
                    iseg_stream_t stream);
int iseg_sgd_momentum_step(float* w, const float* g, float* m, void* w_bf16, const int32_t* seg_of_block, const float* seg_lr_mult,
                           const float* seg_l2, const float* hp, float momentum, int nesterov, const float* seg_sq, float clipnorm,
                           const float* global_sq, float global_clipnorm, int64_t nblocks, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * utils/op_utils.py:43-60 replace_nan_or_inf (layers/fpn.py:52): NaN -> nan_value, then clip to the [min, max] of the
 * tensor with +-inf counted as 0.  ws: 8 bytes.  Gradient passes where x is finite.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_replace_nan_or_inf(const void* x, void* y, int64_t n, float nan_value, int dtype, void* ws, size_t ws_bytes,
                            iseg_stream_t stream);
int iseg_replace_nan_or_inf_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * layers/groupnorm.py:148-207 GroupNormalization (axis=-1): x [N,HW,C], moments over (HW, C/G) per (n, g);
 * mean, rstd [N*G].  layers/rmsnorm.py:22-29 RMSNormalization: y = x * rsqrt(mean_c(x^2)+eps) * (1+scale), rstd [rows].
 * --------------------------------------------------------------------------------------------------------- */
int iseg_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int N, int HW,
                       int C, int G, float eps, int dtype, iseg_stream_t stream);
size_t iseg_groupnorm_bwd_workspace_bytes(int N, int C);
int iseg_groupnorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                       float* dgamma, float* dbeta, int accumulate_param_grads, int N, int HW, int C, int G, int dtype, void* ws,
                       size_t ws_bytes, iseg_stream_t stream);
int iseg_rmsnorm_fwd(const void* x, const float* scale, void* y, float* rstd, int64_t rows, int C, float eps, int dtype,
                     iseg_stream_t stream);
size_t iseg_rmsnorm_bwd_workspace_bytes(int64_t rows, int C);
int iseg_rmsnorm_bwd(const void* dy, const void* x, const float* scale, const float* rstd, void* dx, float* dscale,
                     int accumulate_param_grads, int64_t rows, int C, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Global Response Normalization of ConvNeXt V2: backbones/convnext_v2.py:17-60 GlobalResponseNormlizationLayer.call,
 *   gx[n,c] = sqrt(sum_hw x^2 + eps);  nx = gx / (mean_c gx + eps);  y = gamma*(x*nx) + beta + x      (fp32 arithmetic, output in x's dtype)
 * x, y [N,HW,C] bf16 or fp32 (C % 8 == 0); gamma, beta [C] fp32; nx, gx [N,C] fp32 are written by the forward and read by the backward.
 * The backward returns dx and (+)= dgamma, dbeta; `mul` (NULL, or a tensor shaped like x) multiplies dx elementwise -- the saved derivative of
 * the GELU in front of the layer (Block.call :91-92), so that chain-rule step needs no pass of its own.  One workspace size serves both
 * directions.  All reductions run in a fixed order.
 * --------------------------------------------------------------------------------------------------------- */
size_t iseg_grn_workspace_bytes(int64_t N, int64_t HW, int C);
int iseg_grn_fwd(const void* x, const float* gamma, const float* beta, void* y, float* nx, float* gx, int64_t N, int64_t HW, int C,
                 float eps, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_grn_bwd(const void* dy, const void* x, const float* gamma, const float* nx, const float* gx, const void* mul, void* dx,
                 float* dgamma, float* dbeta, int accumulate_param_grads, int64_t N, int64_t HW, int C, float eps, int dtype, void* ws, size_t ws_bytes,
                 iseg_stream_t stream);
/* The normalisation folded into the Dense that follows it (Block.call :92-93, x = grn(x); x = pwconv2(x)): with a_n = gamma*nx_n + 1 per sample,
 *   grn(g) W + b = g (diag(a_n) W) + (b + beta W),   dW = sum_n diag(a_n) (g_n^T dbr_n) + beta (x) colsum(dbr),
 * and the statistics of the GRN backward follow from the per-sample products g_n^T dbr_n as well -- the passes that would write grn(g) and
 * read it back disappear.  iseg_grn_fwd with y == NULL only computes nx, gx.
 *   iseg_grn_fold_weights: out[n][o][k] = wt[o][k] * a_n[k]    (wt: the K-contiguous bf16 kernel copy [Cout][C4]; out feeds iseg_gemm's B per row group)
 *   iseg_grn_fold_bias:    out[c] = b[c] + sum_k beta[k] W[k][c]                      (W: the fp32 kernel [C4][Cout])
 *   iseg_grn_fold_wgrad:   slabs [N*slabs_per_sample][C4][Cout] fp32 = g^T dbr of consecutive equal row chunks (a batched iseg_gemm), S = colsum(dbr):
 *                          dW (+)= sum_n a_n (.) G_n + beta (x) S;  dstats [N][2*C4] = (sum_hw dz*g | sum dz in row 0, zeros below)
 *   iseg_grn_bwd_folded:   iseg_grn_bwd with those statistics given (dstats is overwritten): no pass over dy for them */
int iseg_grn_fold_weights(const void* wt, const float* gamma, const float* nx, void* out, int64_t N, int Cout, int C4, iseg_stream_t stream);
int iseg_grn_fold_bias(const float* W, const float* beta, const float* b, float* out, int C4, int Cout, iseg_stream_t stream);
int iseg_grn_fold_wgrad(const float* slabs, int slabs_per_sample, const float* W, const float* gamma, const float* beta, const float* nx,
                        const float* S, float* dW, float* dstats, int accumulate, int64_t N, int C4, int Cout, iseg_stream_t stream);
int iseg_grn_bwd_folded(const void* dy, const void* x, const float* gamma, const float* nx, const float* gx, const void* mul, float* dstats,
                        void* dx, float* dgamma, float* dbeta, int accumulate_param_grads, int64_t N, int64_t HW, int C, float eps, int dtype,
                        void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * keras MaxPooling2D(3, strides=2, "same") backbones/resnet_common.py:215-217 and tf.nn.avg_pool2d(..., "SAME")
 * backbones/resnet_blocks.py:182-186.  mode 0 = max (gradient to the first maximal cell), 1 = average over valid cells.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_pool2d_fwd(const void* x, void* y, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int pad_t, int pad_l,
                    int Ho, int Wo, int mode, int dtype, iseg_stream_t stream);
/* relu(a + b), n % 8 == 0: residual join of backbones/resnet_blocks.py:106-107,202-203 */
int iseg_add_relu(const void* a, const void* b, void* y, int64_t n, int dtype, iseg_stream_t stream);
/* max mode with C % 8 == 0 runs two vector passes through a one-byte-per-output-element winner table (workspace); everything else
   takes the one-pass gather kernel and needs no workspace (ws may be NULL when iseg_pool2d_bwd_workspace_bytes returns 0) */
size_t iseg_pool2d_bwd_workspace_bytes(int N, int Ho, int Wo, int C, int mode);
int iseg_pool2d_bwd(const void* x, const void* dy, void* dx, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int pad_t,
                    int pad_l, int Ho, int Wo, int mode, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Attention pieces around the strided-batch GEMMs (iseg_gemm with batch > 1):
 *   softmax over keys of scores [problems, Tq, ld] (cols valid, pad columns written as 0) with the additive terms of
 *   backbones/swin.py:131-158 -- bias [heads,Tq,cols] fp32 (problem z uses head z % heads) and shift mask [windows,Tq,cols]
 *   fp32 (window (z / heads) % windows) -- and the optional probability clip of layers/multihead_self_attention.py:138
 *   (clip_hi > clip_lo enables it).  Backward: dS = P * (g - sum_j g_j P_j), g = dP where the clip passed.
 *   Keras MultiHeadAttention (backbones/vit.py:142-147) uses the same kernels without bias / mask / clip.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_softmax_rows_fwd(const void* scores, void* probs, int64_t problems, int Tq, int cols, int ld, const float* bias, int heads,
                          const float* mask, int windows, float clip_lo, float clip_hi, int dtype, iseg_stream_t stream);
int iseg_softmax_rows_bwd(const void* probs, const void* dprobs, void* dscores, int64_t rows, int cols, int ld, float clip_lo,
                          float clip_hi, int dtype, iseg_stream_t stream);
/* tf.clip_by_value and its gradient (passes where lo <= x <= hi) */
int iseg_clip_fwd(const void* x, void* y, int64_t n, float lo, float hi, int dtype, iseg_stream_t stream);
int iseg_clip_bwd(const void* x, const void* dy, void* dx, int64_t n, float lo, float hi, int dtype, iseg_stream_t stream);
/* y[r,:] = idx[r] >= 0 ? x[idx[r],:] : 0 -- tf.pad / tf.roll / window_partition / window_reverse / crop of
 * backbones/swin.py:46-64,258-288 and PatchMerging's 2x2 space-to-depth (:316-327) as one row permutation each */
int iseg_gather_rows(const void* x, const int32_t* idx, void* y, int64_t rows_in, int64_t rows_out, int C, int dtype,
                     iseg_stream_t stream);
/* y[r,:] = residual[r,:] + scale[g] * (idx[r] >= 0 ? x[idx[r],:] : 0), g = (scale_by_source_row ? idx[r] : r) / rows_per_group; residual
 * and scale optional, C % 8 == 0 -- window_reverse + roll back + crop + drop path + skip connection of a Swin block
 * (backbones/swin.py:264-279, utils/drops.py:8-22) in one pass, and its gradient towards the window rows (inverse table,
 * scale_by_source_row = 1) */
int iseg_gather_rows_fma(const void* x, const int32_t* idx, const float* scale, int64_t rows_per_group, int scale_by_source_row,
                         const void* residual, void* y, int64_t rows_out, int C, int dtype, iseg_stream_t stream);
/* backbones/swin.py:134-142: bias[h,i,j] = table[index[i,j], h]; gradient dtable[k,h] (+)= sum_{index[i,j]==k} dbias[h,i,j]
 * (dbias rows have stride ld) */
/* out[c] (+)= sum_r x[r*ldx + c] for a short, very wide matrix (the [windows, heads*T*ld] score gradients -> bias gradient) */
size_t iseg_colsum_wide_workspace_bytes(int64_t rows, int64_t cols);
int iseg_colsum_wide(const void* x, int64_t ldx, int64_t rows, int64_t cols, float* out, int accumulate, int dtype, void* ws,
                     size_t ws_bytes, iseg_stream_t stream);
int iseg_relpos_bias_gather(const float* table, const int32_t* index, float* bias, int heads, int TT, iseg_stream_t stream);
int iseg_relpos_bias_scatter_grad(const float* dbias, int ld, const int32_t* index, float* dtable, int entries, int heads, int T,
                                  int accumulate, iseg_stream_t stream);
/* the same gradient when `index` is the canonical square-window table of backbones/swin.py:93-104 (window side ws, T = ws*ws,
 * (2ws-1)^2 entries): displacement-enumerating kernel, no table scan */
int iseg_relpos_bias_scatter_grad_window(const float* dbias, int ld, float* dtable, int ws, int heads, int accumulate,
                                         iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * layers/dcn_v3/op.py:16-109 dcnv3_op + utils.py:14-209 (reference points, dilation grids, bilinear sampler), restated
 * exactly (see csrc/dcnv3.hip for the formulae and the [y,x]-vs-[x,y] quirk).  x [N,H,W,G*Cg] (unpadded; `pad` zero ring is
 * implicit), offset [N,Ho,Wo,G*kh*kw*2], mask [N,Ho,Wo,G*kh*kw] (already soft-maxed), y [N,Ho,Wo,G*Cg].
 * Backward: dx_f32 [N,H,W,G*Cg] fp32 (written in full, no need to clear it); doffset / dmask in the storage dtype.  Group widths 8 and
 * 16 (InternImage: 16) take the deterministic path -- int64 fixed-point LDS windows per (output tile, group), then an ordered gather --
 * and need iseg_dcnv3_bwd_workspace_bytes(...) of scratch (0 = the fallback path, which scatters with fp32 atomics, is taken).
 * --------------------------------------------------------------------------------------------------------- */
int iseg_dcnv3_fwd(const void* x, const void* offset, const void* mask, void* y, int N, int H, int W, int G, int Cg, int kh, int kw,
                   int stride, int dil, int pad, float offset_scale, int dtype, iseg_stream_t stream);
size_t iseg_dcnv3_bwd_workspace_bytes(int N, int H, int W, int G, int Cg, int kh, int kw, int stride, int dil, int pad, float offset_scale);
int iseg_dcnv3_bwd(const void* x, const void* offset, const void* mask, const void* dy, float* dx_f32, void* doffset, void* dmask,
                   int N, int H, int W, int G, int Cg, int kh, int kw, int stride, int dil, int pad, float offset_scale, int dtype,
                   void* ws, size_t ws_bytes, iseg_stream_t stream);
/* The same two entry points with the offsets and the mask (and their gradients) as column ranges of ONE [pixels][ld] matrix -- the output of the
 * layer's offset and mask projections (layers/dcn_v3/dcn_v3.py:116-123, two Dense layers on the same input) run as a single product:
 * ld_off / ld_mask = elements between the runs of consecutive output pixels (0 = dense: 2 G P / G P; ld_off even).
 * iseg_dcn_mask_softmax_fwd / _bwd: the softmax over each (pixel, group)'s P mask logits (dcn_v3.py:121-123) in place on columns
 * [col0, col0 + G P) of such a matrix; the backward also clears the columns behind col0 + G P of the gradient matrix (padding up to the
 * product's width), P <= 9.  iseg_split_cols_accumulate: dst0 [rows][n0] += src[:, :n0], dst1 [rows][n1] += src[:, n0:n0+n1] (fp32) -- the
 * joint weight / bias gradient handed back to the two layers. */
int iseg_dcnv3_fwd_ld(const void* x, const void* offset, const void* mask, int64_t ld_off, int64_t ld_mask, void* y, int N, int H, int W, int G,
                      int Cg, int kh, int kw, int stride, int dil, int pad, float offset_scale, int dtype, iseg_stream_t stream);
/* _bwd_ld further takes the storage type of dx (ISEG_F32, or ISEG_BF16: the input gradient is written in the activations' type, no fp32 image
 * and cast pass) and, optionally, a caller-kept side buffer of iseg_dcnv3_bwd_side_bytes(...) bytes that is ALL ZERO on entry and is left all zero
 * (the per-call zeroing of 8 bytes per input element goes away; null = the side buffer lives in `ws` and is zeroed per call). */
size_t iseg_dcnv3_bwd_side_bytes(int N, int H, int W, int G, int Cg, int kh, int kw, int stride, int dil, int pad, float offset_scale);
int iseg_dcnv3_bwd_ld(const void* x, const void* offset, const void* mask, int64_t ld_off, int64_t ld_mask, const void* dy, void* dx, int dx_dtype,
                      void* doffset, void* dmask, int N, int H, int W, int G, int Cg, int kh, int kw, int stride, int dil, int pad,
                      float offset_scale, int dtype, void* ws, size_t ws_bytes, void* side_keep, size_t side_keep_bytes, iseg_stream_t stream);
int iseg_dcn_mask_softmax_fwd(void* om, int64_t pixels, int G, int P, int64_t ld, int col0, int dtype, iseg_stream_t stream);
int iseg_dcn_mask_softmax_bwd(const void* om, void* dom, int64_t pixels, int G, int P, int64_t ld, int col0, int dtype, iseg_stream_t stream);
int iseg_split_cols_accumulate(const float* src, int64_t rows, int64_t ld, float* dst0, int n0, float* dst1, int n1, iseg_stream_t stream);
/* Centre-feature scale of the DCNv3 layer (layers/dcn_v3/dcn_v3.py:138-146; intern_image_huge): out = x (1 - s) + x_proj s with
 * s [pixels, G] (the un-squashed output of center_feature_scale_proj) broadcast over the Cg channels of its group; backward: dx, dx_proj and
 * ds [pixels, G] = sum_c dout (x_proj - x).  Cg in {8, 16}. */
int iseg_dcn_center_blend_fwd(const void* x, const void* x_proj, const void* scale, void* out, int64_t pixels, int G, int Cg, int dtype,
                              iseg_stream_t stream);
int iseg_dcn_center_blend_bwd(const void* dout, const void* x, const void* x_proj, const void* scale, void* dx, void* dx_proj, void* dscale,
                              int64_t pixels, int G, int Cg, int dtype, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * layers/deformable_multihead_self_attention.py:89-244 (compute_attention_internal behind the projections): tanh-bounded offsets (:203-207),
 * softmax over each head's P points (:210-214), clipped sampling positions (:225-230), the four gather_nd of _bilinear_sample with weights from
 * the unclipped floor (:124-169) and the weighted sum over the points (:236-240) as ONE launch, no intermediate tensor.
 * value [N,H,W,heads*Ch], offset_logits [N,H,W,heads*P*2] (raw, read as [heads, P, (y, x)]), attn_logits [N,H,W,heads*P] (raw), out [N,H,W,heads*Ch];
 * 1 <= P <= 16 (otherwise ISEG_ERR_UNSUPPORTED), any heads and Ch (Ch % 8 == 0 with 16-byte aligned value / out takes the 16-byte-load route).
 * tanh, softmax, coordinates and weights in fp32 whatever the storage dtype.
 * Backward (the gradient of the same lines): from the three operands and dout, dvalue / doffset_logits / dattn_logits in the storage dtype; tanh and
 * softmax are recomputed.  dvalue is accumulated by int64 2^-40 fixed-point atomics (order-free: bit-identical from run to run) in `ws`, at least
 * iseg_defattn_bwd_workspace_bytes(...) bytes, 16-byte aligned, zeroed by the call; a non-finite contribution makes the whole dvalue NaN.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_defattn_fwd(const void* value, const void* offset_logits, const void* attn_logits, void* out, int N, int H, int W, int heads, int P, int Ch,
                     float offset_range_factor, int dtype, iseg_stream_t stream);
size_t iseg_defattn_bwd_workspace_bytes(int N, int H, int W, int heads, int Ch);
int iseg_defattn_bwd(const void* value, const void* offset_logits, const void* attn_logits, const void* dout, void* dvalue, void* doffset_logits,
                     void* dattn_logits, int N, int H, int W, int heads, int P, int Ch, float offset_range_factor, int dtype, void* ws,
                     size_t ws_bytes, iseg_stream_t stream);

/* out[c] (+)= sum_r a[r][c]*b[r][c]: gradient of the per-channel layer scale x * gamma (backbones/intern_image/
 * intern_image_layer.py:128,136,160,168) */
int iseg_scale_cols(const void* x, const float* colscale, void* y, int64_t rows, int C, int dtype, iseg_stream_t stream);
size_t iseg_mul_colsum_workspace_bytes(int64_t rows, int C);
int iseg_mul_colsum(const void* a, const void* b, int64_t rows, int C, float* out, int accumulate, int dtype, void* ws,
                    size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fused window attention (backbones/swin.py:117-167 WindowAttention.call between the qkv and proj Dense layers):
 *   out[b,:,h] = softmax(scale * q k^T + bias[h] + mask[b % mask_windows]) v    for qkv [windows, T, 3*heads*32] bf16
 * bias [heads,T,T] fp32 (iseg_relpos_bias_gather) and mask [mask_windows,T,T] fp32 (or NULL) are first folded into one padded
 * additive table (iseg_window_attention_table).  One wavefront per (window, head), MFMA
 * for all five products, nothing of size T x T in HBM.  Supported: bf16, head_dim 32, T <= 64 (iseg_window_attention_supported).
 * Backward recomputes the probabilities; dbias [heads,T,T] fp32 is overwritten (sum over windows, fixed order).
 * --------------------------------------------------------------------------------------------------------- */
int iseg_window_attention_supported(int T, int head_dim, int dtype);
/* table[w][h][64][64] fp32 = bias[h] + mask[w] inside T x T, -FLT_MAX outside (w < mask_windows; one window when mask is NULL) */
int iseg_window_attention_table(const float* bias, const float* mask, float* table, int T, int heads, int mask_windows,
                                iseg_stream_t stream);
int iseg_window_attention_fwd(const void* qkv, const float* table, void* out, int64_t windows, int T, int heads, int table_windows,
                              float scale, int dtype, iseg_stream_t stream);
size_t iseg_window_attention_bwd_workspace_bytes(int64_t windows, int T, int heads);
int iseg_window_attention_bwd(const void* qkv, const float* table, const void* dout, void* dqkv, float* dbias, int64_t windows, int T,
                              int heads, int table_windows, float scale, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Forward-only global self-attention for inference (keras MultiHeadAttention of backbones/vit.py:142-147,166 under
 * core_inference.py's sliding windows): out[b,:,h] = softmax(scale * q k^T) v for packed qkv [batch, T, 3*heads*64] bf16.
 * Online softmax over key tiles of 64: no T x T tensor in HBM.  Supported: bf16, head_dim 64, any T.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_attention_fwd_supported(int head_dim, int dtype);
int iseg_attention_fwd(const void* qkv, void* out, int64_t batch, int T, int heads, int head_dim, float scale, int dtype,
                       iseg_stream_t stream);
/* Training pair of the same kernel family (same support set).  The forward additionally returns, per (sample, head, token) and
 * padded to a multiple of 64 tokens (iseg_attention_lse_elems floats), log2 of the softmax denominator in the kernel's exp2 domain;
 * the backward recomputes the probabilities from qkv and that vector, tile by tile (dQ kernel over key tiles, dK/dV kernel over
 * query tiles: no atomics, fixed summation order).  dqkv has the layout of qkv and is overwritten; workspace = one float per
 * lse element. */
size_t iseg_attention_lse_elems(int64_t batch, int T, int heads);
int iseg_attention_fwd_train(const void* qkv, void* out, float* lse2, int64_t batch, int T, int heads, int head_dim, float scale,
                             int dtype, iseg_stream_t stream);
size_t iseg_attention_bwd_workspace_bytes(int64_t batch, int T, int heads);
int iseg_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse2, void* dqkv, int64_t batch, int T,
                       int heads, int head_dim, float scale, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Attention core of the single-head non-local block, layers/self_attention.py:65-93 (between the 1x1 projections and the feature
 * dropout) with get_attention of utils/attention_utils.py:23-40: out[b] = softmax(scale * q[b] k[b]^T) v[b] for a 64-wide query /
 * key and a wide value.  q, k [batch, T, dk]; v, out, dout [batch, T, dv]; every operand has its own row pitch in elements (ld*),
 * the sample stride is T * pitch -- column ranges of one packed projection output or separate tensors; q and k may be the same
 * pointer (shared_querykey).  Online softmax over key tiles of 64, one wavefront per (sample, 64-query tile, 64-column value slab):
 * no T x T tensor in HBM.  Supported (iseg_self_attention_supported): bf16, dk == 64, dv % 64 == 0, 64 <= dv <= 1024; any T >= 1;
 * pitches that are multiples of 8 elements and cover their rows, 16-byte aligned bases, scale > 0.  Anything else returns
 * ISEG_ERR_UNSUPPORTED before any memory is touched.
 * layers/self_attention.py:65-93, utils/attention_utils.py:23-40 -- forward: lse2 NULL for inference; for training it receives, per
 * (sample, token) and padded to a multiple of 64 tokens (iseg_self_attention_lse_elems floats, zeros in the padding), log2 of the
 * softmax denominator in the kernel's exp2 domain. */
int iseg_self_attention_supported(int dk, int dv, int dtype);
/* layers/self_attention.py:65-93, utils/attention_utils.py:23-40 -- floats in lse2, and in the dsum vector of the backward call */
size_t iseg_self_attention_lse_elems(int64_t batch, int T);
int iseg_self_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo,
                            float* lse2, int64_t batch, int T, int dk, int dv, float scale, int dtype, iseg_stream_t stream);
/* layers/self_attention.py:65-93, utils/attention_utils.py:23-40 -- gradient of the same lines: the probabilities are recomputed from
 * q, k and lse2, tile by tile (dV per (key tile, value slab), dQ per query tile, dK per key tile: no atomics, fixed summation order, a
 * second run is bit-identical).  dsum is caller-owned scratch of iseg_self_attention_lse_elems floats (overwritten: row dots of
 * dout and out over all dv columns).  dq, dk, dv are overwritten; dq and dk are always separate buffers -- when q and k alias, the
 * caller adds the two. */
int iseg_self_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* out,
                            int64_t ldo, const void* dout, int64_t lddo, const float* lse2, float* dsum, void* dq, int64_t lddq, void* dk,
                            int64_t lddk, void* dv, int64_t lddv, int64_t batch, int T, int dk_dim, int dv_dim, float scale, int dtype,
                            iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * On-device input pipeline: data_process/pipeline.py:85-170 (StandardAugmentationsPipeline, training branch) + data_process/input_norm.py:7-80
 * as one gather per output pixel -- random scale (bilinear image / nearest label, utils.py:303-370), bottom / right pad with the mean
 * pixel / ignore label (augments/pad_augment.py), random crop, random flip, random erasing with noise (augments/random_erasing_augment.py)
 * and out = v * norm_scale[c] + norm_shift[c].  images [B, Hs, Ws, 3] float32 (dtype 0) or uint8 (dtype 2), zero-padded to a common size;
 * labels [B, Hs, Ws] int32 or NULL; params [B, iseg_augment_params_ints()] int32 on the device, per sample:
 * H, W (valid source size), newH, newW (after the scale), off_y, off_x (crop offset in the scaled + padded image), flip, n_erase (<= 5),
 * then n_erase x (y, x, h, w) in output coordinates.  The host draws them; the device only draws the erase noise (seed).
 * Optional photometric table fparams [B, iseg_augment_params_floats()] float32 (NULL = none; round 3), per sample: brightness delta
 * (augments/random_brightness_augment.py: + delta, clip [0, 256]; 0 = not executed), contrast factor (tf.image.adjust_contrast about the
 * channel means in slots 2..4, which iseg_augment_channel_means fills from the scaled + brightness-adjusted image; 1 = not executed),
 * saturation factor (1) and hue delta (0) (augments/random_photo_metric_distortions.py: contrast -> saturation -> hue -> clip), and the
 * stddev of RandomNoisyEvalAugment's N(0, sigma) noise (evaluation pipeline: added after the padding, clip [0, 256]).  The photometric
 * steps sit between the random scale and the padding (pipeline.py:129-134): pad and erased pixels are not touched by them.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_augment_params_ints(void);
int iseg_augment_params_floats(void);
size_t iseg_augment_means_workspace_bytes(int B);
int iseg_augment_channel_means(const void* images, int image_dtype, const int32_t* params, float* fparams, int B, int Hs, int Ws, void* ws,
                               size_t ws_bytes, iseg_stream_t stream);
int iseg_augment_crop_batch(const void* images, int image_dtype, const int32_t* labels, const int32_t* params, const float* fparams,
                            const float* mean_pixel, const float* norm_scale, const float* norm_shift, int ignore_label, float* out_images,
                            int32_t* out_labels, int B, int Hs, int Ws, int crop_h, int crop_w, uint64_t seed, iseg_stream_t stream);
int iseg_normalize_image(const float* x, float* y, int64_t pixels, const float* norm_scale, const float* norm_shift, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * augments/random_rotate_augment.py:20-115 (transform = tf.raw_ops.ImageProjectiveTransformV3) and :221-296 (random_rotated_inputs) for a
 * padded batch in one launch, CONSTANT fill mode only.  images [B][Hs][Ws][C] fp32, C in 1..4; labels [B][Hs][Ws] int32 or NULL (with
 * out_labels); transforms [B][8] = a0 a1 a2 b0 b1 b2 c0 c1 on the device, mapping the OUTPUT (x, y) to the INPUT point
 * x' = ((a0 x + a1 y) + a2) / k, y' = ((b0 x + b1 y) + b2) / k, k = c0 x + c1 y + 1 (k == 0 -> fill), fp32 without FMA contraction (bit-equal
 * to a float32 restatement in this order); sizes [B][2] int32 on the device = (H, W) of each sample in the top-left corner of its Hs x Ws slot,
 * NULL = (Hs, Ws).  image_interp 0: nearest at (lround(y'), lround(x')), half away from zero; 1: bilinear over floor / floor + 1 with weights
 * (xc - x'), (x' - xf), every tap outside the sample's own H x W reading image_fill.  Labels are always nearest with label_fill.  Bounds are
 * tested on the float coordinate (huge / NaN = outside).  replace [C] (host) or NULL: out < -1e-6 ? replace[c] : out, the reference's tf.where
 * after a fill of -1 (border pixels blend with -1 first: a 0 that blends to -1e-5 IS replaced).  Output positions outside a sample's (H, W)
 * get replace (image_fill when NULL) and label_fill.  ISEG_ERR_UNSUPPORTED for C outside 1..4 or another image_interp.
 * One departure from TensorFlow's arithmetic: a bilinear pixel none of whose four taps lies inside the sample is image_fill itself.  TF evaluates
 * the weighted sum there too, which is image_fill up to rounding for ordinary coordinates but 0 for |x'| or |y'| >= 2^24, where its fp32
 * weights xc - x' and x' - xf both round to 0.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_projective_transform_batch(const float* images, const int32_t* labels, const float* transforms, const int32_t* sizes,
                                    float* out_images, int32_t* out_labels, int B, int Hs, int Ws, int C, int image_interp, float image_fill,
                                    const float* replace, int label_fill, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fused logits tail of the training step: tf.image.resize(bilinear) of the low-resolution logits z [N,Hi,Wi,C] to the label size
 * (layers/core_model_ext.py:199-256) + the ignore-label cross-entropy mean and its gradient w.r.t. z
 * (losses/catecrossentropy_ignore_label.py:44-88) + the argmax confusion matrix (metrics/seg_metric_wrapper.py:89-102), in one pass that
 * never writes the [N,Ho,Wo,C] fp32 logits or their gradient.  Same arithmetic as iseg_resize_bilinear_fwd followed by
 * iseg_softmax_ce_confusion followed by iseg_resize_bilinear_bwd (TF's lerp order, first-max argmax, zero one-hot row for labels
 * outside [0,C)), deterministic.  Needs an integer factor (rows even, columns a power of two <= 64) and C <= 32
 * (iseg_upsample_ce_supported); other shapes take the three separate calls.
 *   loss_sum[0] = loss_sum_scale * sum_p w_p (logsumexp(l_p) - l_p[y_p]);  dz (same dtype as z, or NULL) = grad_scale * d(sum)/dz;
 *   cm [C,C] uint64 (or NULL) += counts.
 * --------------------------------------------------------------------------------------------------------- */
int iseg_upsample_ce_supported(int Hi, int Wi, int Ho, int Wo, int C);
size_t iseg_upsample_ce_workspace_bytes(int N, int Hi, int Wi, int Ho, int Wo, int C);
int iseg_upsample_ce(const void* z, int dtype, const int32_t* labels, const float* class_w, int N, int Hi, int Wi, int Ho, int Wo, int C,
                     int ignore_label, float* loss_sum, float loss_sum_scale, void* dz, float grad_scale, uint64_t* cm, void* ws,
                     size_t ws_bytes, iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the matrix cores: keras.layers.Conv2D(filters, k, strides, padding="same", dilation_rate,
 * groups, use_bias) as built by layers/model_builder.py:54-64 (ConvNormAct.conv), layers/aspp.py:41-52 (dilated 3x3 branches),
 * backbones/resnet_blocks.py:175-205, backbones/convnext.py:72-75,255-257 (2x2/s2 or dilated downsample), layers/simpledecoder.py:21-36.
 * x [N,H,W,Cin], w [KH,KW,Cin/groups,Cout] (Keras layout, bf16 shadow), y [N,Ho,Wo,Cout]; pt / pl = TF "same" top / left padding
 * (the halo is zero chunks of the gathered operand -- no padded copy, no [pixels, KH*KW*Cin] column buffer, no col2im scatter).
 * bf16 storage, channels per group multiples of 8 (iseg_conv2d_igemm_supported); fp32 parity runs keep iseg_im2col + iseg_gemm.
 *   fwd         y = conv(x, w) (+ bias)
 *   bwd_data    dx = conv^T(dy, w)          gather form, deterministic
 *   bwd_weight  dw (+)= x^T * dy per tap    fp32 [KH,KW,Cin/groups,Cout], fixed-order split-K slabs
 * Workspace (split-K slabs): iseg_conv2d_igemm_workspace_bytes(geom, pass) with pass 0 fwd, 1 bwd_data, 2 bwd_weight,
 * 3 = iseg_conv2d_patch_bwd_weight (below).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct iseg_conv_geom {
    int N, H, W, Cin, Cout, KH, KW, sh, sw, dh, dw, pt, pl, Ho, Wo, groups;
} iseg_conv_geom;
int iseg_conv2d_igemm_supported(const iseg_conv_geom* geom_h, int dtype);
size_t iseg_conv2d_igemm_workspace_bytes(const iseg_conv_geom* geom_h, int pass);
int iseg_conv2d_igemm_fwd(const void* x, const void* w, const float* bias, void* y, const iseg_conv_geom* geom_h, int dtype, void* ws,
                          size_t ws_bytes, iseg_stream_t stream);
/* The forward pass on the LDS-DMA pipeline (csrc/conv_igemm_dma.h): `wt` is the K-contiguous copy [Cout][KH*KW*Cin] of the Keras kernel (what
 * iseg_transpose_batched keeps per weight update); one group, Cin % 64 == 0, Cout % 8 == 0.  iseg_conv2d_igemm_bwd_data takes the same pipeline by
 * itself for stride-1 problems with Cout % 64 == 0 (the Keras kernel already is K-contiguous for that product). */
int iseg_conv2d_igemm_fwd_kt_supported(const iseg_conv_geom* g, int dtype);
int iseg_conv2d_igemm_fwd_kt(const void* x, const void* wt, const float* bias, void* y, const iseg_conv_geom* g, int dtype, void* ws,
                             size_t ws_bytes, iseg_stream_t stream);
int iseg_conv2d_igemm_bwd_data(const void* dy, const void* w, void* dx, const iseg_conv_geom* geom_h, int dtype, void* ws, size_t ws_bytes,
                               iseg_stream_t stream);
int iseg_conv2d_igemm_bwd_weight(const void* x, const void* dy, float* dw, int accumulate, const iseg_conv_geom* geom_h, int dtype, void* ws,
                                 size_t ws_bytes, iseg_stream_t stream);

/* Patchify convolutions (kernel == stride, dilation 1, one group, H % KH == 0, W % KW == 0, pt = pl = 0: backbones/convnext.py:72-75, the 2x2 /
 * stride-2 downsampling layers) as plain GEMMs over a patch view of the NHWC tensor (csrc/conv_patchify.hip): the [pixels, KH*KW*Cin] patch
 * matrix is the tensor itself with a grouped row stride and KH contiguous K segments of KW*Cin elements, so nothing is gathered or scattered.
 *   fwd         y = P wt^T (+ bias)   wt = the K-contiguous kernel copy [Cout][KH*KW*Cin]; LDS-DMA GEMM with a patch-view A
 *   bwd_data    dx = dy w^T           w = the Keras kernel; the product iseg_gemm runs for the column buffer, stored at the pixels (same bits
 *                                     as iseg_gemm + iseg_col2im)
 *   bwd_weight  dw (+)= P^T dy, dbias (+)= column sums of dy (NULL: not wanted)   fp32, the weight-gradient LDS-DMA GEMM with iseg_gemm's
 *                                     split rule and fixed-order slab sum; needs iseg_conv2d_igemm_workspace_bytes(geom, 3)
 * iseg_conv2d_patch_supported(geom, dtype, pass): pass 0 / 1 / 2 as above -- bf16, KW*Cin % 8 == 0, Cout % 8 == 0, the LDS-DMA GEMM's own
 * conditions for the pass's M, N, K without a reduction split (fwd also: KW*Cin a multiple of the K-step, 64 or 32; bwd_weight: the
 * conditions of iseg_gemm_variant 7 / 8, >= 2048 output pixels).  The passes are independent; fwd and bwd_data need no workspace (ws may be NULL).
 * 16-byte aligned operands; anything else returns ISEG_ERR_UNSUPPORTED. */
int iseg_conv2d_patch_supported(const iseg_conv_geom* geom_h, int dtype, int pass);
int iseg_conv2d_patch_fwd(const void* x, const void* wt, const float* bias, void* y, const iseg_conv_geom* geom_h, int dtype, void* ws,
                          size_t ws_bytes, iseg_stream_t stream);
int iseg_conv2d_patch_bwd_data(const void* dy, const void* w, void* dx, const iseg_conv_geom* geom_h, int dtype, void* ws, size_t ws_bytes,
                               iseg_stream_t stream);
int iseg_conv2d_patch_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int accumulate, const iseg_conv_geom* geom_h, int dtype,
                                 void* ws, size_t ws_bytes, iseg_stream_t stream);

/* Several convolutions of ONE input [N,H,W,Cin] -- layers/aspp.py:33-52, the pixel-level 1x1 and the dilated 3x3 branches: stride 1, "same"
 * padding, one group, Cout filters each, their own kernel size / dilation -- as one launch per pass (csrc/conv_igemm_dma.h):
 *   fwd         blockIdx.z = branch: y_b = conv(x, w_b) (+ bias_b), written at column y_col of rows of ldy elements
 *   bwd_data    dx = sum_b conv^T(dy_b, w_b) (+ residual) as ONE product whose reduction runs over (branch, tap, channel): the branch
 *               gradients meet in the fp32 accumulators and are rounded once
 *   bwd_weight  blockIdx.z = branch: gw_b (+)= x^T * dy_b per tap, one pass over the pixels, no slabs
 * A branch lists the operands of all three passes; a pass reads only its own.  bf16 storage, Cin % 64 == 0, Cout % 64 == 0, N*H*W >= 64
 * (iseg_conv2d_branches_supported), 16-byte aligned operands, leading dimensions multiples of 8; anything else returns ISEG_ERR_UNSUPPORTED.
 * Workspace: fwd and bwd_weight need none (their branches fill the chip; ws may be NULL).  bwd_data is one stride-1 data gradient whose taps
 * are the taps of every branch in a row, and may split that reduction: iseg_conv2d_igemm_workspace_bytes(g, 1) with g = {N, H, W, Cin, Cout,
 * KH = 1, KW = sum of KH_b * KW_b, strides and dilations 1, pt = pl = 0, Ho = H, Wo = W, groups = 1}. */
#define ISEG_CONV_MAX_BRANCHES 4
typedef struct iseg_conv_branch {
    int KH, KW, dh, dw, pt, pl;
    const void* wt;          /* fwd: K-contiguous kernel copy [Cout][KH*KW*Cin] */
    const void* w;           /* bwd_data: Keras kernel [KH,KW,Cin,Cout] */
    const float* bias;       /* fwd, may be NULL */
    void* y;                 /* fwd: output rows */
    int64_t ldy, y_col;
    const void* dy;          /* bwd_data, bwd_weight: gradient rows of lddy elements */
    int64_t lddy;
    float* gw;               /* bwd_weight: fp32 [KH,KW,Cin,Cout] */
} iseg_conv_branch;
typedef struct iseg_conv_branches {
    int N, H, W, Cin, Cout, count;
    iseg_conv_branch b[ISEG_CONV_MAX_BRANCHES];
} iseg_conv_branches;
int iseg_conv2d_branches_supported(const iseg_conv_branches* t, int dtype);
int iseg_conv2d_branches_fwd(const void* x, const iseg_conv_branches* t, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);
int iseg_conv2d_branches_bwd_data(const iseg_conv_branches* t, void* dx, const void* residual, int64_t ldr, int dtype, void* ws, size_t ws_bytes,
                                  iseg_stream_t stream);
int iseg_conv2d_branches_bwd_weight(const void* x, const iseg_conv_branches* t, int accumulate, int dtype, void* ws, size_t ws_bytes,
                                    iseg_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fused ConvNeXt MLP (backbones/convnext.py:51-63 Block.call: pwconv1 -> act (exact GELU) -> pwconv2 -> gamma -> drop_path ->
 * + input) for the wide stages, bf16 storage, C = 96 / 192 (iseg_convnext_mlp_supported):
 *     out[m][:] = residual[m][:] + rowscale[m / rows_per_group] * gamma[:] * (gelu(y2[m][:] @ W1 + b1) @ W2 + b2)
 * y2 = LayerNorm output [M, C].  The [M, 4C] hidden tensor never reaches HBM in the forward pass and is recomputed by the backward
 * chain.  The kernels stream the weights as bf16 *tiled* images (the byte order of their LDS ring stages):
 *   iseg_convnext_mlp_prep      fp32 Keras kernels W1 [C, 4C], W2 [4C, C] (+ layer scale gamma [C] or NULL) -> fw_tiled
 *                               (iseg_convnext_mlp_tiled_bytes(C, 0) bytes) and, when bw_tiled != NULL, bw_tiled (.. (C, 1) bytes; it
 *                               holds W1, W2 * gamma and W1 again in the orders the backward products read them); once per step
 *   iseg_convnext_mlp_fwd       the formula above; gamma / rowscale (per-sample drop-path factor) may be NULL
 *   iseg_convnext_mlp_bwd       dbr [M, C] = rowscale * d(out)  ->  g [M, 4C] = gelu(h), dh [M, 4C] = (dbr @ (W2 gamma)^T) * gelu'(h)
 *                               (the operands of the two weight-gradient GEMMs) and dy2 [M, C] = dh @ W1^T
 * --------------------------------------------------------------------------------------------------------- */
int iseg_convnext_mlp_supported(int C, int dtype);
size_t iseg_convnext_mlp_tiled_bytes(int C, int backward);
int iseg_convnext_mlp_prep(const float* W1, const float* W2, const float* gamma, void* fw_tiled, void* bw_tiled, int C,
                           iseg_stream_t stream);
/* all per-weight-update derivations of a model's ConvNeXt blocks in one launch.  table (device): per entry 8 x int64
 * {kind, p1, p2, p3, p4, p5, n, rows}: kind 1 = iseg_convnext_mlp_prep(W1 = p1, W2 = p2, gamma = p3 | 0, fw_tiled = p4, bw_tiled = p5 | 0, C = n);
 * kind 0 = iseg_scale_cols_cast(src = p1, colscale = p3, dst(bf16) = p4, rows, cols = n).  max_elements sizes the grid. */
int iseg_convnext_weight_prep_batched(const int64_t* table, int entries, int64_t max_elements, iseg_stream_t stream);
int iseg_convnext_mlp_fwd(const void* y2, const void* fw_tiled, const float* b1, const float* b2, const float* gamma,
                          const float* rowscale, int64_t rows_per_group, const void* residual, void* out, int64_t M, int C, int dtype,
                          iseg_stream_t stream);
int iseg_convnext_mlp_bwd(const void* y2, const void* dbr, const void* bw_tiled, const float* b1, void* g, void* dh, void* dy2,
                          int64_t M, int C, int dtype, iseg_stream_t stream);
/* The same block's backward pass with NO [M, 4C] tensor in HBM (round 3; the training path uses this pair):
 *   iseg_convnext_mlp_bwd_data  dy2 [M, C] only; dbr = rowscale[m / rows_per_group] * dout is formed while the rows are loaded
 *                               (rowscale may be NULL); mean != NULL: `y` is the LayerNorm input y1, normalised on load like in _wgrad
 *   iseg_convnext_mlp_wgrad     every parameter gradient of backbones/convnext.py:51-57 (pwconv1, pwconv2, gamma), ACCUMULATED into
 *                               dW1 [C, 4C], db1 [4C], dW2 [4C, C], db2 [C], dgamma [C]: workgroups own 128 hidden units and a chunk of
 *                               rows, recompute gelu(h) / dh for them and contract over the rows on the matrix cores; partial sums per
 *                               row chunk in `ws` (iseg_convnext_mlp_wgrad_workspace_bytes), summed in chunk order by a second launch
 *                               (deterministic).  With gamma: dW2 += (g^T dbr) gamma, dgamma += sum_k W2 o (g^T dbr) + b2 S,
 *                               db2 += gamma S with S = column sums of dbr; gamma == NULL: dW2 += g^T dbr, db2 += S.  W2 / b2 / gamma
 *                               are the fp32 masters.  mean != NULL: `y` is the LayerNorm INPUT y1 and y2 = (y1 - mean) rstd ln_gamma +
 *                               ln_beta is formed while the rows are staged.  rowscale needs rows_per_group % 64 == 0. */
int iseg_convnext_mlp_bwd_data(const void* y, const float* mean, const float* rstd, const float* ln_gamma, const float* ln_beta,
                               const void* dout, const float* rowscale, int64_t rows_per_group, const void* bw_tiled, const float* b1,
                               void* dy2, int64_t M, int C, int dtype, iseg_stream_t stream);

/* The same chain carried through the LayerNorm in front of the MLP as well (LayerNorm on the row load, backbones/convnext.py:26-27,52): y1 is the
 * LayerNorm INPUT, dy1 receives its gradient -- rstd (t - mean_c(t) - xhat mean_c(t xhat)), t = dy2 gamma -- and the column sums
 * dgamma += sum_rows dy2 xhat, dbeta += sum_rows dy2 are added to dln_gamma / dln_beta (per-workgroup partial rows in ws, fixed-order sum;
 * deferred when a reduction queue is open).  Replaces iseg_convnext_mlp_bwd_data + iseg_layernorm_bwd for the fused stages. */
size_t iseg_convnext_mlp_bwd_data_ln_workspace_bytes(int64_t M, int C);
int iseg_convnext_mlp_bwd_data_ln(const void* y1, const float* mean, const float* rstd, const float* ln_gamma, const float* ln_beta,
                                  const void* dout, const float* rowscale, int64_t rows_per_group, const void* bw_tiled, const float* b1,
                                  void* dy1, float* dln_gamma, float* dln_beta, int64_t M, int C, int dtype, void* ws, size_t ws_bytes,
                                  iseg_stream_t stream);
/* the forward kernel with keras.layers.LayerNormalization(epsilon) (backbones/convnext.py:27,49) folded into its row load: y1 = the
 * depthwise convolution's output; mean / rstd [M] are written for the backward kernels; y2 never exists in HBM */
int iseg_convnext_mlp_fwd_ln(const void* y1, const float* ln_gamma, const float* ln_beta, float eps, float* mean, float* rstd,
                             const void* fw_tiled, const float* b1, const float* b2, const float* gamma, const float* rowscale,
                             int64_t rows_per_group, const void* residual, void* out, int64_t M, int C, int dtype, iseg_stream_t stream);
size_t iseg_convnext_mlp_wgrad_workspace_bytes(int64_t M, int C);
int iseg_convnext_mlp_wgrad(const void* y, const float* mean, const float* rstd, const float* ln_gamma, const float* ln_beta,
                            const void* dout, const float* rowscale, int64_t rows_per_group, const void* bw_tiled, const float* b1,
                            const float* W2, const float* b2, const float* gamma, float* dW1, float* db1, float* dW2, float* db2,
                            float* dgamma, int64_t M, int C, int dtype, void* ws, size_t ws_bytes, iseg_stream_t stream);

/* The pair above in ONE pass over the rows at C = 96 (iseg_convnext_mlp_bwd_data_ln + iseg_convnext_mlp_wgrad recompute the [M, 4C] hidden
 * tile twice; here a workgroup owns a chunk of rows and all 384 hidden units and forms it once): dy1 [M, C] = the gradient of the LayerNorm
 * INPUT y1, dln_gamma / dln_beta += the LayerNorm parameter gradients, dW1 / db1 / dW2 / db2 / dgamma += the MLP parameter gradients -- the
 * argument set and the semantics are the union of the two calls (LayerNorm on the row load is mandatory: mean, rstd, ln_gamma, ln_beta).
 * dh feeds dy2 with the derivative of the sigmoid-form GELU (the chain kernel's polynomial differs by <= 8.7e-4 before the bf16 rounding).
 * No atomics: per-chunk records in ws, fixed-order sums.  The workspace is sized by iseg_convnext_mlp_wgrad_workspace_bytes(M, 96): the two
 * launchers leave the same chunk records and share one size function, which answers the larger need (this one's 256 chunks).  The LayerNorm
 * partial rows are deferred when a reduction queue is open.  rowscale needs rows_per_group % 64 == 0. */
int iseg_convnext_mlp_bwd_onepass(const void* y1, const float* mean, const float* rstd, const float* ln_gamma, const float* ln_beta,
                                  const void* dout, const float* rowscale, int64_t rows_per_group, const void* bw_tiled, const float* b1,
                                  const float* W2, const float* b2, const float* gamma, void* dy1, float* dln_gamma, float* dln_beta,
                                  float* dW1, float* db1, float* dW2, float* db2, float* dgamma, int64_t M, int C, int dtype, void* ws,
                                  size_t ws_bytes, iseg_stream_t stream);

/* Gemma text backbone (nlp/gemma).
 * iseg_gemma_rope: rotary embedding of nlp/gemma/gemma_attention.py:96-114 on the packed projection rows qkv [rows = B * T][(nq + 2 nkv) h] =
 *   [q heads | k heads | v heads] (row pitches ld_in / ld_out in elements; out == qkv: in place).  Per q / k head, with x1 = x[0:h/2], x2 = x[h/2:h]:
 *   out[2i] = x1[i] cos - x2[i] sin, out[2i+1] = x2[i] cos + x1[i] sin (the reference's stack(..., axis=-1) + reshape: INTERLEAVED).  The v columns
 *   are copied unchanged.  table fp32 [T][h] = [sin(t / 10000^(2i/h)), i < h/2 | cos(...)]; fp32 arithmetic, one rounding.  inverse = 1 applies
 *   the transposed rotation (the backward pass: out[i] = g[2i] cos + g[2i+1] sin, out[h/2+i] = g[2i+1] cos - g[2i] sin). */
int iseg_gemma_rope(const void* qkv, int64_t ld_in, void* out, int64_t ld_out, const float* table, int64_t rows, int T, int nq, int nkv, int h,
                    int inverse, int dtype, iseg_stream_t stream);
/* nlp/gemma/gemma_attention.py:116-151, gemma_decoder_block.py:114-136 -- causal grouped-query attention with a key-side padding mask:
 *   out[b,t,n,:] = sum_s softmax_s(scale * q[b,t,n,:] . k[b,s,n / (nq/nkv),:]) v[b,s,n / (nq/nkv),:], over the keys s <= t with padding_mask[b,s] != 0.
 * q / out / dout / dq [batch, T, nq h], k / v / dk / dv [batch, T, nkv h]: column ranges of a packed buffer or separate tensors, each with its
 * row pitch in elements; padding_mask one byte per (b, s) or NULL (all visible).  The nq/nkv query heads of one key/value head are stacked as
 * (nq/nkv) T query rows of one problem (row t * (nq/nkv) + j); online softmax over key tiles of 64, key tiles wholly above the diagonal are
 * skipped, the value width is walked in slabs of 64 columns.  Nothing of size T x T is stored, no atomics, fixed summation order.  A query
 * row with no visible key gives out = 0, lse2 = 0 and dq = 0; masked pairs contribute exactly 0 to dk and dv.
 * Supported (iseg_gemma_attention_supported): bf16, h % 64 == 0, 64 <= h <= 256, nq % nkv == 0; any T >= 1; pitches multiples of 8 covering
 * their rows, 16-byte aligned bases, scale > 0.  Anything else returns ISEG_ERR_UNSUPPORTED before any memory is touched.
 * lse2 (NULL for inference) and the dsum scratch of the backward call hold iseg_gemma_attention_lse_elems floats: per (sample, key/value head)
 * the stacked rows padded to a multiple of 64. */
int iseg_gemma_attention_supported(int nq, int nkv, int h, int dtype);
size_t iseg_gemma_attention_lse_elems(int64_t batch, int T, int nq, int nkv);
int iseg_gemma_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const uint8_t* padding_mask,
                             void* out, int64_t ldo, float* lse2, int64_t batch, int T, int nq, int nkv, int h, float scale, int dtype,
                             iseg_stream_t stream);
/* gradient of the same lines; dq, dk, dv are overwritten (dk / dv already summed over the query heads of each group, in stacked-row order) */
int iseg_gemma_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const uint8_t* padding_mask,
                             const void* out, int64_t ldo, const void* dout, int64_t lddo, const float* lse2, float* dsum, void* dq,
                             int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, int64_t batch, int T, int nq, int nkv, int h,
                             float scale, int dtype, iseg_stream_t stream);
/* nlp/gemma/gemma_backbone.py:152 -- gradient of the token-embedding lookup: dtable[id,:] += scale * sum over the n tokens with that id of dy[token,:],
 * added in increasing token order.  sorted_ids [n] = the ids in stable ascending order, order [n] = the token each came from (both int64, a
 * stable sort of the ids); dy [n, d] in `dtype`, dtable fp32 [vocab, d].  One workgroup per run of equal ids owns its row: rows of
 * absent ids are not touched, no atomics. */
int iseg_embedding_grad(const void* dy, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n, int64_t vocab, int d,
                        float scale, int dtype, iseg_stream_t stream);
/* Gemma with a key/value cache (nlp/gemma/gemma_causal.py:186-226).  A cache is a base pointer, a batch stride and a row pitch in elements: row s
 * of sample b starts at base + b * batch_stride + s * pitch and holds nkv h elements; one layer's key (value) slice of the reference's
 * [B, num_layers, 2, S, nkv, h] cache is such a view.
 * iseg_gemma_rope_cache: nlp/gemma/gemma_attention.py:161-179 -- the rotary embedding at the positions pos0 + t and the dynamic_update_slice of
 *   the cache.  Reads the packed projection rows qkv [batch * Tn][(nq + 2 nkv) h]; writes the rotated q heads to q_out [batch * Tn][nq h] (pitch
 *   ldq), the rotated k heads to row pos0 + t of kcache and the unchanged v heads to row pos0 + t of vcache.  table is iseg_gemma_rope's, fp32
 *   [S][h]; the output is interleaved and rounded once, bit for bit iseg_gemma_rope's.  bf16 and fp32.  Cache rows outside
 *   [pos0, pos0 + Tn) are not written; pos0 < 0 or pos0 + Tn > S returns ISEG_ERR_ARG before anything is touched. */
int iseg_gemma_rope_cache(const void* qkv, int64_t ld_in, void* q_out, int64_t ldq, void* kcache, int64_t k_batch, int64_t ldk, void* vcache,
                          int64_t v_batch, int64_t ldv, const float* table, int64_t batch, int S, int pos0, int Tn, int nq, int nkv, int h,
                          int dtype, iseg_stream_t stream);
/* nlp/gemma/gemma_attention.py:116-151 under the mask of gemma_decoder_block.py:114-136 with a cache (no padding mask: compute_causal_mask alone):
 *   out[b,t,n,:] = sum_{s <= pos0 + t} softmax_s(scale * q[b,t,n,:] . K[b,s,n / (nq/nkv),:]) V[b,s,n / (nq/nkv),:]
 * for the Tn new tokens at positions pos0 .. pos0 + Tn - 1; q / out [batch, Tn, nq h] with their row pitches.  The (nq/nkv) * Tn query rows of one
 * (sample, key/value head) are stacked (row t * (nq/nkv) + j).  Pass 1, one workgroup per (sample, key/value head, chunk): the visible keys are
 * cut into `splits` chunks of whole 64-key tiles, each walked with the online softmax; per stacked row an fp32 partial (maximum, sum, h
 * accumulators) goes to the workspace.  Pass 2 merges the partials in chunk order and rounds once to bf16.  No atomics: a second call is
 * bit-identical.  Keys past pos0 + Tn - 1 are never loaded: the cache behind the write position may hold anything.
 * splits: 0 = the launcher's plan, a function of (batch, pos0, Tn, nkv) alone that iseg_gemma_decode_attention_splits returns; a positive value
 * is taken, clipped to the number of 64-key tiles that hold a visible key.  The workspace holds iseg_gemma_decode_attention_scratch_bytes
 * (same `splits` argument); a smaller one returns ISEG_ERR_WORKSPACE.
 * Supported (iseg_gemma_decode_attention_supported): bf16, h % 64 == 0, 64 <= h <= 256, nq % nkv == 0, (nq/nkv) * Tn <= 16; scale > 0, pitches
 * and batch strides multiples of 8 elements, 16-byte aligned bases.  Anything else returns ISEG_ERR_UNSUPPORTED, and pos0 < 0 or
 * pos0 + Tn > S returns ISEG_ERR_ARG, before any memory is touched. */
int iseg_gemma_decode_attention_supported(int Tn, int nq, int nkv, int h, int dtype);
int iseg_gemma_decode_attention_splits(int64_t batch, int pos0, int Tn, int nq, int nkv, int h);
size_t iseg_gemma_decode_attention_scratch_bytes(int64_t batch, int pos0, int Tn, int nq, int nkv, int h, int splits);
int iseg_gemma_decode_attention(const void* q, int64_t ldq, const void* kcache, int64_t k_batch, int64_t ldk, const void* vcache, int64_t v_batch,
                                int64_t ldv, void* out, int64_t ldo, void* ws, size_t ws_bytes, int64_t batch, int S, int pos0, int Tn, int nq,
                                int nkv, int h, float scale, int splits, int dtype, iseg_stream_t stream);
/* The same two launchers with the position in DEVICE memory: pos_d is one int32, shared by the batch, that the kernels read when they run, so a
 * captured graph of a decoding step can be replayed at every position (GemmaCausalLM.compile(graph_decode=True)).  All other arguments are those
 * of iseg_gemma_rope_cache / iseg_gemma_decode_attention.
 * iseg_gemma_rope_cache_at: for 0 <= *pos_d <= S - Tn, q_out and the cache rows are bit for bit iseg_gemma_rope_cache's at pos0 = *pos_d.
 * iseg_gemma_decode_attention_at: the same supported set.  The grid cannot depend on the position, so it is the plan of the cache's capacity,
 *   pos0 = S - Tn, and the workspace holds iseg_gemma_decode_attention_scratch_bytes(batch, S - Tn, Tn, nq, nkv, h, splits) bytes: the chunk
 *   count and the scratch size never decrease with pos0, so what suffices at the capacity suffices at every position.  Every workgroup derives
 *   from *pos_d the tile count and the effective chunk count that iseg_gemma_decode_attention plans on the host for that position (the same
 *   functions, compiled for both sides); pass-1 workgroups whose chunk index is at or past the effective count return at once and pass 2
 *   merges the effective chunks alone, in chunk order.  For 0 <= *pos_d <= S - Tn the output is therefore bit for bit
 *   iseg_gemma_decode_attention(pos0 = *pos_d, same `splits`), splits = 0 included.  Keys past *pos_d + Tn - 1 are never loaded.
 * The host cannot check a device value: with *pos_d outside [0, S - Tn] every workgroup of both launchers returns without reading or writing any
 * memory other than *pos_d.  Everything the host can check is refused before any memory is touched with the codes above: pitches, alignment,
 * the supported set (ISEG_ERR_UNSUPPORTED), a null or misaligned pos_d and Tn > S (ISEG_ERR_ARG), a short workspace (ISEG_ERR_WORKSPACE). */
int iseg_gemma_rope_cache_at(const void* qkv, int64_t ld_in, void* q_out, int64_t ldq, void* kcache, int64_t k_batch, int64_t ldk, void* vcache,
                             int64_t v_batch, int64_t ldv, const float* table, int64_t batch, int S, const int32_t* pos_d, int Tn, int nq, int nkv,
                             int h, int dtype, iseg_stream_t stream);
int iseg_gemma_decode_attention_at(const void* q, int64_t ldq, const void* kcache, int64_t k_batch, int64_t ldk, const void* vcache, int64_t v_batch,
                                   int64_t ldv, void* out, int64_t ldo, void* ws, size_t ws_bytes, int64_t batch, int S, const int32_t* pos_d, int Tn,
                                   int nq, int nkv, int h, float scale, int splits, int dtype, iseg_stream_t stream);
/* The commit of one decoding step: the tail of the body of sample_loop (iseg_amd/nlp/samplers.py:21-39, keras_nlp Sampler.__call__) and the head of
 * its next iteration, on state in device memory; one launch of one workgroup that loops over the rows (any batch).
 *   prompt [batch, S] ids and cur_ids [batch] of type ids_dtype, tokens [batch] (the sampler's choice) of type tokens_dtype: ISEG_IDS_I32 or
 *   ISEG_IDS_I64;  mask [batch, S] one byte per entry, non-zero = user token;  done [batch] bytes;  row pitches in elements;
 *   pos_d one int32: the index of the previous token (generate_step's cache_update_index = index - 1);  end_token_id < 0: none.
 * With p = *pos_d, read by every thread before a barrier:
 *   freeze   if p + 1 is outside [0, S), or end_token_id >= 0 and every done[b] is set, nothing is written: samplers.py:30 (`while index <
 *            max_length`) and :31-34 (the break once every row is done).  A replay after the generation has ended changes nothing.
 *   commit   otherwise, per row:  t = mask[b, p+1] ? prompt[b, p+1] : tokens[b] converted to ids_dtype (:36-37);  prompt[b, p+1] = t;
 *            cur_ids[b] = t (the token the next step embeds, :35 through generate_step's `next`);
 *            done[b] |= (t == end_token_id && !mask[b, p+1]);  then, after a barrier, one thread writes *pos_d = p + 1 (:38).
 * With the initial done[b] = any_s(prompt[b, s] == end_token_id && !mask[b, s]) computed by the caller (:32) this is sample_loop, provided an end
 * token that a not-yet-generated, non-user position holds at the start is not the row's only one to be overwritten before the loop ends: `done`
 * here only ever turns on, :32 is recomputed from the prompt (GemmaCausalLM.generate_step checks this on the host and otherwise runs the loop).
 * The all-done reduction goes through LDS; plain loads and stores, no atomics. */
#define ISEG_IDS_I32 0
#define ISEG_IDS_I64 1
int iseg_decode_commit(void* prompt, int64_t ld_prompt, const uint8_t* mask, int64_t ld_mask, int32_t* pos_d, void* cur_ids, uint8_t* done,
                       const void* tokens, int64_t batch, int S, int64_t end_token_id, int ids_dtype, int tokens_dtype, iseg_stream_t stream);
/* The samplers behind GemmaCausalLM.compile(sampler=) (nlp/gemma/gemma_causal.py class docstring: keras_nlp.samplers Random / TopK / TopP): one
 * token id per row of logits [batch, V] (bf16 or fp32, row pitch ld >= V elements) from ONE uniform u[b] in [0, 1) per row that the caller
 * draws; no random numbers are made here.  tokens int32 [batch].  Per row x, in exact arithmetic (the kernels work in fp32):
 *   order      x descending, then index ascending; NaN above +inf above the finite values above -inf, -0 ties with +0.  The order is taken on
 *              the STORED values (not on x / T), so ties are the input's.
 *   non-finite if the first of the order is NaN, +inf or -inf (all masked) its index is the token -- the lowest index holding the top value,
 *              torch.argmax's answer -- and u is not read.  Otherwise -inf entries weigh 0 and are never drawn.
 *   weights    w_i = exp(x_i / T - max_j x_j / T), W = sum_i w_i, T = temperature > 0.
 *   kept set   ISEG_SAMPLE_RANDOM: every index.  ISEG_SAMPLE_TOP_K: the first min(k, V) of the order.  ISEG_SAMPLE_TOP_P: among the first
 *              k' = min(k, V) of the order (k = 0: V), position j iff the weights of the positions before it sum to <= p W (the full softmax
 *              mass, not a renormalised one); the first is always kept.
 *   draw       the kept ids in TOKEN-ID order, S = their weight: the token is the smallest kept id i whose cumulative kept weight up to and
 *              including i exceeds u S; if rounding leaves none, the largest kept id with a weight > 0.  Ids with weight 0 are never returned.
 * Pass 1, one workgroup per (row, chunk of whole 2048-element tiles): the chunk's top key (a monotone integer image of the stored value) with
 * its lowest index, the chunk's weight sum relative to its own maximum and, for TOP_K / TOP_P, 256-bin histograms of counts and of mass over the
 * top key digit, mass as fixed-point integers so that the sums do not depend on the order of the additions.  Pass 2, one workgroup per row,
 * merges the partials in chunk order, finds the cut key by radix selection (the remaining digits from filtered sweeps of the row) and how many
 * of the elements tied with it are kept, lowest index first, then draws with prefix sums over the row as stored.  No atomics across
 * workgroups: a second call returns the same tokens.  128-bit loads when logits is 16-byte aligned and ld * element size is a multiple of 16,
 * scalar loads otherwise.
 * splits: 0 = the launcher's plan, a function of (batch, V) alone that iseg_token_sample_splits returns; a positive value is taken, clipped to
 * the number of 2048-element tiles that hold an element.  The scratch buffer (8-byte aligned) holds iseg_token_sample_scratch_bytes (same
 * `splits` argument); a smaller one returns ISEG_ERR_WORKSPACE.
 * Supported (iseg_token_sample_supported): bf16 or fp32, 1 <= V <= 2^20, k >= 0, k >= 1 for TOP_K (k > V is V); anything else returns
 * ISEG_ERR_UNSUPPORTED.  temperature <= 0 or not finite, p outside (0, 1] and ld < V return ISEG_ERR_ARG.  All before any memory is touched. */
#define ISEG_SAMPLE_RANDOM 0
#define ISEG_SAMPLE_TOP_K 1
#define ISEG_SAMPLE_TOP_P 2
int iseg_token_sample_supported(int64_t V, int mode, int k, int dtype);
int iseg_token_sample_splits(int64_t batch, int64_t V);
size_t iseg_token_sample_scratch_bytes(int64_t batch, int64_t V, int mode, int k, int splits);
int iseg_token_sample(const void* logits, int64_t ld, const float* u, int32_t* tokens, void* ws, size_t ws_bytes, int64_t batch, int64_t V, int mode,
                      int k, float p, float temperature, int splits, int dtype, iseg_stream_t stream);
/* One step of keras_nlp.samplers.BeamSampler (GemmaCausalLM.compile(sampler=BeamSampler(num_beams=2)) in the class docstring of
 * nlp/gemma/gemma_causal.py) without a [rows, V] intermediate and without a second cache.  rows = groups * nb: row g * nb + j is beam j of batch
 * row g, 1 <= nb <= 16.
 *
 * iseg_beam_select: logits [rows, V] (bf16 or fp32, row pitch ld >= V elements), log_probs fp32 [rows] (the running scores), T = temperature > 0.
 *   score      of (beam j, token v) of a group, in exact arithmetic:  (x[j, v] - max_u x[j, u]) / T - log sum_u exp((x[j, u] - max x[j]) / T)
 *              + log_probs[j], evaluated directly (not as log(softmax)): a candidate whose fp32 softmax underflows to 0 keeps its true score
 *              and its place in the order, where the reference gets -inf and an arbitrary one.
 *   selection  per group the nb best of the nb * V candidates with flat index j * V + v:  parents[g nb + r] = j, tokens[g nb + r] = v,
 *              new_log_probs[g nb + r] = the score, r = 0 .. nb - 1 sorted by score descending, ties by flat index ascending.  Within one row the
 *              score order is the order of the STORED logits (value descending, then index ascending: order_keys.h), and a row's candidates
 *              are its nb first in that order; the rows' candidates are then ranked by their rounded fp32 scores.
 *   non-finite a -inf logit scores -inf.  A row that holds a NaN or a +inf logit, or -inf alone, scores NaN throughout (as log_softmax does), and so
 *              does a row whose log_probs is NaN; NaN ranks above every number, as in torch.topk, so such a row's candidates are its tokens
 *              0 .. min(nb, V) - 1.  Whatever the input, 0 <= parents < nb and 0 <= tokens < V, and the nb pairs of a group are distinct.
 *   accuracy   the exponent (x - m) log2(e) / T is formed in fp64 and split into an fp32 head and tail, v_exp_f32 takes the head and the tail
 *              enters linearly: a weight is off by at most 2 * 2^-23 of itself whatever its exponent.  Weights are summed in fp64 in a fixed
 *              order; the score is formed in fp64 and rounded once.  |score error| <= 2 * 2^-23 + 2^-24 |score|.
 * Pass 1, one workgroup per (row, chunk of whole 2048-element tiles), reads the logits ONCE: the chunk's nb first entries of the order with
 * their indices and, relative to the chunk's own maximum, the sum of the weights.  Pass 2, one workgroup per group and one wavefront per row:
 * merges the row's chunk records in a fixed order (each sum scaled by exp((m_chunk - m_row) / T), as the decode merge), takes the row's nb first
 * entries, forms their scores, and the first wavefront selects nb of the <= nb * nb candidates.  No atomics across workgroups: a second call
 * returns the same bits.  128-bit loads when logits is 16-byte aligned and ld * element size is a multiple of 16, scalar loads otherwise.
 * splits: 0 = the launcher's plan, a function of (rows, V) alone that iseg_beam_select_splits returns; a positive value is taken, clipped to
 * the number of 2048-element tiles that hold an element.  The scratch buffer (8-byte aligned) holds iseg_beam_select_scratch_bytes (same
 * `splits` argument); a smaller one returns ISEG_ERR_WORKSPACE.  Supported (iseg_beam_select_supported): bf16 or fp32, 1 <= V <= 2^20,
 * 1 <= nb <= 16; anything else returns ISEG_ERR_UNSUPPORTED.  rows that are no multiple of nb, a temperature <= 0 or not finite and ld < V
 * return ISEG_ERR_ARG.  All before any memory is touched.
 *
 * iseg_beam_reorder: keras_nlp's gather_beams by `parents` (int32 [groups * nb], device memory) IN PLACE, on the cache and on the prompt.
 *   cache      [groups * nb, planes, Sc, row_bytes] bytes, contiguous (planes = num_layers * 2, Sc positions of its own, which need not be
 *              the prompt's S; row_bytes = nkv * head_dim * element size, a multiple of 16; base 16-byte aligned):  cache[g nb + j, p, s] = old cache[g nb + parents[g nb + j], p, s] for s < len only;
 *              positions >= len are neither read nor written.  The gather moves data between the beams of one group at identical
 *              coordinates, so one thread owns a 16-byte column across the nb beams: it loads the source of every j with parents[j] != j, then
 *              stores them.  No other thread touches those addresses: no second cache, no barrier, any mapping (several children of one
 *              parent included).  A group of identity parents costs no access to the cache at all.  cache NULL or len 0: skipped.
 *   prompt     [groups * nb, S] ids (int32 or int64, row pitch ld_prompt elements), mask [groups * nb, S] bytes (row pitch ld_mask), tokens
 *              int32 [groups * nb]:  prompt[g nb + j, :] = old prompt[g nb + parents[g nb + j], :], then prompt[r, index] = tokens[r] unless
 *              mask[r, index] marks a user token (the mask is not gathered: the beams of a group share it).  One thread owns a column of
 *              the group here too.  prompt NULL: skipped.
 * A group with a parent outside [0, nb) is left untouched, cache and prompt.  Grid-stride launches; no host read.  nb outside 1 .. 16, a
 * row_bytes that is no multiple of 16, a misaligned cache, len outside [0, Sc], index outside [0, S) and a row pitch below S return
 * ISEG_ERR_ARG, before any memory is touched. */
int iseg_beam_select_supported(int64_t V, int nb, int dtype);
int iseg_beam_select_splits(int64_t rows, int64_t V);
size_t iseg_beam_select_scratch_bytes(int64_t rows, int64_t V, int nb, int splits);
int iseg_beam_select(const void* logits, int64_t ld, const float* log_probs, int32_t* parents, int32_t* tokens, float* new_log_probs, void* ws,
                     size_t ws_bytes, int64_t rows, int64_t V, int nb, float temperature, int splits, int dtype, iseg_stream_t stream);
int iseg_beam_reorder(void* cache, int64_t planes, int64_t Sc, int64_t row_bytes, int64_t len, void* prompt, int64_t S, int64_t ld_prompt,
                      const uint8_t* mask, int64_t ld_mask, const int32_t* tokens, int64_t index, int ids_dtype, const int32_t* parents, int64_t groups,
                      int nb, iseg_stream_t stream);
/* One step of keras_nlp.samplers.ContrastiveSampler (contrastive search) without a [B, V] probability tensor, without a [B k, T] similarity
 * matrix and without copying or gathering a cache.  Row b * k + j is candidate j of batch row b (groups = B), 1 <= k <= 16.
 *
 * iseg_contrastive_candidates: logits [R, V] (bf16 or fp32, row pitch ld >= V elements), T = temperature > 0 -> probs fp32 [rows, k] and tokens
 * int32 [rows, k]: the k largest of p = softmax(x / T) of every output row and their token ids.
 *   row map    row_map NULL: R = rows and output row r reads logits row r.  Otherwise int32 [rows] in device memory and R = rows * group: output
 *              row r reads logits row r * group + row_map[r] (clamped into [0, group)), so a step reads the previous step's winner out of its
 *              [B k, V] logits and never gathers it.
 *   order      probability descending, ties by token id ascending: the order of the STORED logits (value descending, then index ascending;
 *              order_keys.h), which is the probabilities' order wherever two of them differ.  The reference's top_k(sorted=False) has none.
 *   precision  p = exp((x - max) / T) / sum_u exp((x_u - max) / T): the weights as iseg_beam_select forms them (each within 2 * 2^-23 of itself),
 *              summed in fp64 in a fixed order; the candidate's own weight and the quotient in fp64, rounded once to fp32:
 *              |error| <= 2.5 * 2^-23 p.  The reference rounds the probabilities to the logits' dtype; here they stay fp32.
 *   non-finite a -inf logit has p = 0.  A row whose largest entry is NaN or +inf, or that holds -inf alone, has p = NaN throughout (as softmax
 *              has) and, every token tying, the tokens 0 .. k - 1.  Whatever the input, 0 <= token < V and a row's k tokens are distinct.
 * Pass 1 is iseg_beam_select's (one workgroup per (row, chunk of whole 2048-element tiles), the logits read ONCE); pass 2, one wavefront per
 * output row, merges the chunk records.  No atomics: a second call returns the same bits.  splits, the scratch buffer (8-byte aligned,
 * iseg_contrastive_candidates_scratch_bytes with the same `splits`; smaller: ISEG_ERR_WORKSPACE) and the plan
 * (iseg_contrastive_candidates_splits(rows, V)) are iseg_beam_select's.  Supported (iseg_contrastive_candidates_supported): bf16 or fp32,
 * 1 <= V <= 2^20, 1 <= k <= min(16, V); anything else returns ISEG_ERR_UNSUPPORTED.  A temperature <= 0 or not finite, ld < V and a row map
 * with group < 1 return ISEG_ERR_ARG.  All before any memory is touched.
 *
 * iseg_contrastive_select: hist [groups, S, D] the hidden states of the positions so far (bf16 or fp32; batch stride hs_b and position stride
 * hs_t in elements), index the number of filled positions, cand [groups * k, D] the candidates' hidden states (row pitch ldc), probs fp32
 * [groups * k], 0 <= alpha <= 1 -> max_sim fp32 [groups * k], scores fp32 [groups * k], winner int32 [groups]:
 *   max_sim[b k + j] = max over t < index of  <hist[b, t], cand[b k + j]> / (|hist[b, t]| * |cand[b k + j]|),
 *   scores[b k + j]  = (1 - alpha) * probs[b k + j] - alpha * max_sim[b k + j],      winner[b] = the first j with the maximal score.
 *   arithmetic the dot product and the two squared norms are fp32 FMA chains over the stored elements (8 consecutive elements per lane and
 *              512-element trip, then a 64-lane butterfly), square roots, one product and one division in fp32.  No epsilon: a zero vector in
 *              the history or as a candidate gives 0 / 0 = NaN, as in the reference.  |error of max_sim| <= (2 D + 8) * 2^-24.
 *   NaN        ranks above every number, as torch.max and torch.argmax have it: one NaN similarity makes max_sim NaN, a NaN score wins.
 *              0 <= winner < k always.
 *   positions  >= index are never read.  1 <= index <= S.
 * Pass 1, one workgroup per (batch row, chunk of positions, group of candidates): the candidates stay in LDS (all k of them where k * D
 * elements fit 128 KB, else groups of equal size and the history is read once per group) while the chunk's positions stream by once; the
 * record is the largest order key of sim per candidate.  Pass 2, one wavefront per batch row, takes the maxima over the chunks and forms scores
 * and winner.  A similarity does not depend on the chunk its position falls into and a maximum does not depend on the grouping: every output
 * is bit-identical for every `splits`, and from call to call.  No atomics.  splits: 0 = the launcher's plan, a function of (groups, index, D, k,
 * dtype) that iseg_contrastive_select_splits returns; a positive value is taken, clipped to `index`.  The scratch buffer (4-byte aligned)
 * holds iseg_contrastive_select_scratch_bytes (same `splits`); smaller: ISEG_ERR_WORKSPACE.  Supported (iseg_contrastive_select_supported):
 * bf16 or fp32, D a multiple of 8 in 8 .. 16384, 1 <= k <= 16; anything else returns ISEG_ERR_UNSUPPORTED.  index outside 1 .. S, alpha
 * outside [0, 1], bases that are not 16-byte aligned, pitches below D or no multiple of 8 elements return ISEG_ERR_ARG, before any memory is
 * touched.
 *
 * iseg_contrastive_commit: the winner's state becomes its group's, IN PLACE, one launch, with w = winner[b] (int32 [groups], device memory):
 *   cache      [groups * k, planes, Sc, row_bytes] bytes, contiguous, as iseg_beam_reorder takes it:  cache[b k + j, p, pos] = cache[b k + w, p,
 *              pos] for every plane p and every j; no other position is read or written.  The rows of a group are equal below pos (the cache
 *              was repeated k times once), so one position per step is all that ever moves.  cache NULL: skipped.
 *   prompt     [groups * k, S] ids (int32 or int64, row pitch ld_prompt):  prompt[b k + j, index] = prompt[b k + w, index].  NULL: skipped.
 *   hist       [groups, Sh, D] as above:  hist[b, index] = cand[b k + w].  NULL: skipped.
 * A thread owns a 16-byte column: it reads the winner's and writes the others'.  A group whose winner lies outside [0, k) is left untouched.
 * Grid-stride launch; no host read.  k outside 1 .. 16, a row_bytes or D * element size that is no multiple of 16, misaligned bases, pos
 * outside [0, Sc), index outside [0, S) or [0, Sh) and a row pitch below the row return ISEG_ERR_ARG, before any memory is touched. */
int iseg_contrastive_candidates_supported(int64_t V, int k, int dtype);
int iseg_contrastive_candidates_splits(int64_t rows, int64_t V);
size_t iseg_contrastive_candidates_scratch_bytes(int64_t rows, int64_t V, int k, int splits);
int iseg_contrastive_candidates(const void* logits, int64_t ld, const int32_t* row_map, int group, float* probs, int32_t* tokens, void* ws,
                                size_t ws_bytes, int64_t rows, int64_t V, int k, float temperature, int splits, int dtype, iseg_stream_t stream);
int iseg_contrastive_select_supported(int64_t D, int k, int dtype);
int iseg_contrastive_select_splits(int64_t groups, int64_t index, int64_t D, int k, int dtype);
size_t iseg_contrastive_select_scratch_bytes(int64_t groups, int64_t index, int64_t D, int k, int splits, int dtype);
int iseg_contrastive_select(const void* hist, int64_t hs_b, int64_t hs_t, int64_t S, int64_t index, const void* cand, int64_t ldc,
                            const float* probs, int32_t* winner, float* scores, float* max_sim, void* ws, size_t ws_bytes, int64_t groups, int64_t D,
                            int k, float alpha, int splits, int dtype, iseg_stream_t stream);
int iseg_contrastive_commit(void* cache, int64_t planes, int64_t Sc, int64_t row_bytes, int64_t pos, void* prompt, int64_t S, int64_t ld_prompt,
                            int64_t index, int ids_dtype, void* hist, int64_t hs_b, int64_t hs_t, int64_t Sh, const void* cand, int64_t ldc, int64_t D,
                            int dtype, const int32_t* winner, int64_t groups, int k, iseg_stream_t stream);
/* The language-model head's loss without a [tokens, vocab] tensor: SparseCategoricalCrossentropy(from_logits=True) and
 * SparseCategoricalAccuracy of nlp/gemma/gemma_causal.py:165-172 on the logits Z = X E^T (X [M, d] hidden states, E [V, d] the tied table).  The
 * caller cuts the vocabulary into chunks [v0, v0 + w) of any width w >= 1, has iseg_gemm write Z_c = X E[v0 : v0 + w]^T [M, w] in FP32 (row pitch
 * ld >= w elements; never rounded to bf16) and hands each chunk to the kernels below.  Rows are independent; t = targets[r] (int32).
 *   state      per row, fp32 m, s, z_t and int32 argmax.  Before the first chunk the caller sets m = -inf, s = 0 (z_t and argmax: anything, 0
 *              is a good choice).  After the chunks that cover [0, V) once each, in increasing v0:  m = max_v Z[r,v];  s = sum_v exp(Z[r,v] - m);
 *              z_t = Z[r,t] if 0 <= t < V, else untouched;  argmax = the SMALLEST v with Z[r,v] = m (ties inside a chunk and across chunks).
 *   chunk_fwd  merges one chunk into the state:  m' = max(m, max_j z_j);  s' = s exp(m - m') + sum_j exp(z_j - m');  z_t = z_{t - v0} when
 *              v0 <= t < v0 + w;  argmax = v0 + (smallest j with z_j = max_j z_j) when that maximum is > m (strictly: an earlier chunk keeps a tie).
 *              exp(-inf - x) is 0 and no difference of two -inf is formed: the empty state and -inf logits cost nothing.
 *   non-finite NaN is never a maximum and never the argmax (comparisons with it are false), but it is summed: one NaN logit in a row makes
 *              s, lse and the loss of THAT row NaN, and every entry of that row of G.  A +inf logit does the same (inf - inf), as softmax does.
 *              A row of -inf alone has lse = -inf and a NaN loss.
 *   finalise   lse[r] = m + log s;  valid = 0 <= t < V;  w_r = valid ? (weights ? weights[r] : 1) : 0;  loss[r] = scale w_r (lse - z_t), evaluated
 *              from the fp32 state in fp64 as log s - (z_t - m) and rounded once (so is lse), and
 *              exactly 0 where w_r = 0 whatever the row holds (the zero row of tf.one_hot, as iseg_softmax_ce_ignore treats a label outside the
 *              classes).  scale is a constant factor of the loss (1, or 1 / tokens for Keras' sum_over_batch_size) that chunk_bwd is given too;
 *              match[r] = valid and argmax = t.  sums[0..2] = sum_r loss[r], sum_r w_r match[r], sum_r w_r: wavefront and workgroup partial sums
 *              in a fixed order, the per-workgroup records (scratch, iseg_lm_head_ce_scratch_bytes(M) bytes, 4-byte aligned; a smaller one
 *              returns ISEG_ERR_WORKSPACE) summed in fp64 by one workgroup.  No atomics: a second call returns the same bits.
 *   chunk_bwd  from the chunk's Z_c computed AGAIN (nothing [M, V] is saved) and the final state's m and s:
 *                  G[r, j] = scale w_r up_r (exp(z_j - lse[r]) - [v0 + j == t]),   j < w,
 *              evaluated as exp(z_j - m) (c_r / s) - [v0 + j == t] c_r with c_r = scale w_r up_r (the rounding of m + log s would move every
 *              probability of the row by half an ulp of lse; z_j - m is exact for neighbouring magnitudes; c_r and c_r / s are rounded once
 *              each), in fp32 and rounded once to `dtype`.  exp is v_exp_f32 on t log2 e = hi + lo with the product's rounding error kept
 *              in lo: one ulp whatever |t| is, in chunk_fwd too (row pitch ldg >= w; columns j >= w are not written).  upstream NULL: up_r = 1.
 *              Rows with w_r = 0 are written as zeros without reading their logits (not NaN * 0).  X^T G and G E[v0 : v0 + w] are iseg_gemm's.
 * One wavefront per row and chunk, 16-byte loads along the row when the base is 16-byte aligned and the pitch a multiple of 16 bytes (both
 * buffers for chunk_bwd), scalar accesses otherwise; the last, narrower chunk and any w that is no multiple of 4 take the scalar path at the
 * row's end only.  Rows are taken in trips of at most 32768 per launch grid.  v0 + w must stay below 2^31 - 1024.  Bad arguments return
 * ISEG_ERR_ARG before any memory is touched.  iseg_lm_head_ce_chunk_default: the chunk width the Python layer uses when none is forced, in
 * [1, V] (0 for V < 1); profiles/lm_head_ce_kbench.md has the sweep behind it. */
int iseg_lm_head_ce_chunk_default(int64_t M, int64_t V);
size_t iseg_lm_head_ce_scratch_bytes(int64_t M);
int iseg_lm_head_ce_chunk_fwd(const float* z, int64_t ld, const int32_t* targets, float* m, float* s, float* zt, int32_t* argmax, int64_t M,
                              int64_t v0, int64_t w, iseg_stream_t stream);
/* z_t[r] = x_r . E[t_r] once more for the rows with 0 <= t < V (the others are not touched): the d products summed in fp64 and rounded once to
 * fp32, in place of the value chunk_fwd took from Z_c.  The loss sets ONE logit against lse, a softmax-weighted average of all of them that
 * smooths the GEMM's accumulation error (d roundings per logit); the single logit carries it whole, and it is what separates the loss from the
 * correctly rounded one at the fp32 compute type.  Call it after the chunks and before finalise; x [M, d] and table [V, d] in `dtype` with
 * their row pitches in elements.  One wavefront per row, 16-byte loads when both bases are 16-byte aligned, both pitches multiples of 16 bytes
 * and d a multiple of 8, scalar loads otherwise. */
int iseg_lm_head_ce_target_logit(const void* x, int64_t ldx, const void* table, int64_t ldt, const int32_t* targets, float* zt, int64_t M, int64_t V,
                                 int64_t d, int dtype, iseg_stream_t stream);
int iseg_lm_head_ce_finalise(const float* m, const float* s, const float* zt, const int32_t* argmax, const int32_t* targets, const float* weights,
                             float* loss, float* lse, int32_t* match, float* sums, void* scratch, size_t scratch_bytes, int64_t M, int64_t V,
                             float scale, iseg_stream_t stream);
int iseg_lm_head_ce_chunk_bwd(const float* z, int64_t ld, const float* m, const float* s, const int32_t* targets, const float* weights,
                              const float* upstream, float scale, void* g, int64_t ldg, int64_t M, int64_t V, int64_t v0, int64_t w, int dtype,
                              iseg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ISEG_HIP_H */
