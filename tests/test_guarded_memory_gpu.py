"""The existing parity tests once more, inside guard-band memory (tests/guarded_memory.py): every workspace is EXACTLY as large as its
iseg_*_workspace_bytes function says and full of NaN, every output kernels.py allocates starts as NaN, operands and outputs sit at addresses
= 16 (mod 512) between 64 KiB bands of poison, and after the body the bands must be untouched.  The oracle, the inputs and the tolerances are
those of the test bodies that are called; nothing is restated here except two short cases for wrappers no test body calls directly.

CASES is also the ledger tests/test_guarded_memory_host.py checks against include/iseg_hip.h: `needs` names the workspace functions a case
must have queried (with a non-zero answer) while it ran."""
import contextlib
import importlib
from collections import namedtuple

import pytest
import torch

from tests import guarded_memory as GM

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
MP = object()      # stands for a MonkeyPatch of the case's own

Case = namedtuple("Case", "id module func args needs refuses prelaunch")
TK, MISC = "tests.test_kernels_gpu", "tests.test_misc_gpu"
HERE = "tests.test_guarded_memory_gpu"


def _dn(d):
    return "f32" if d == F32 else "bf16"


def _cases():
    out = []

    def add(cid, module, func, args, needs=(), refuses="first", prelaunch=False):
        """needs: the workspace functions the body must ask, with a non-zero answer.  refuses: the one whose launcher is the body's FIRST scratch
        user -- run 16 bytes short, that launcher must be the one that refuses (default: needs[0]; None: the body is not run short).
        prelaunch: the refused wrapper launches a kernel of its own before the launcher that needs the scratch"""
        needs = tuple(needs)
        out.append(Case(cid, module, func, tuple(args), needs, (needs[0] if needs else None) if refuses == "first" else refuses, prelaunch))

    gemm, ln, bn = "iseg_gemm_workspace_bytes", "iseg_layernorm_bwd_workspace_bytes", "iseg_bn_workspace_bytes"
    for d in (F32, BF):
        n = _dn(d)
        # ---- GEMM, register-staged --------------------------------------------------------------------------------------------------
        add(f"gemm_fwd-77x21x256-{n}", TK, "test_gemm_forward_orientation", (d, 77, 21, 256))
        add(f"gemm_fwd-33x40x24-{n}", TK, "test_gemm_forward_orientation", (d, 33, 40, 24))
        add(f"gemm_dgrad_gelu-70x21x256-{n}", TK, "test_gemm_dgrad_and_gelu_grad", (d, 70, 21, 256))
        add(f"gemm_wgrad_split3-1030x21x256-{n}", TK, "test_gemm_wgrad_splitk", (d, 1030, 21, 256, 3), [gemm])
        add(f"gemm_wgrad_bias-64x96x21-{n}", TK, "test_wgrad_with_fused_bias_gradient", (d, 64, 96, 21))
        add(f"gemm_strided_concat-{n}", TK, "test_gemm_strided_output_into_concat", (d,))
        # ---- LayerNorm --------------------------------------------------------------------------------------------------------------
        for rows, C in ((7, 8), (1, 96), (129, 768), (203, 2730)):
            add(f"layernorm-{rows}x{C}-{n}", TK, "test_layernorm_fwd_bwd", (d, rows, C), [ln])
        for rows, C, groups in ((7, 8, 1), (520, 112, 4)):
            for flags in ((True, True, True), (False, False, False), (True, False, True)):
                add(f"layernorm_post-{rows}x{C}x{groups}-{''.join('ft'[f] for f in flags)}-{n}", TK, "test_layernorm_post_norm_tail",
                    (d, rows, C, groups) + flags, [ln])
        for rows, C, pad in ((64, 32, 0), (257, 192, 3)):
            add(f"layernorm_gather-{rows}x{C}x{pad}-{n}", TK, "test_layernorm_with_row_tables_and_gather_fma", (d, rows, C, pad), [ln])
        # ---- BatchNorm --------------------------------------------------------------------------------------------------------------
        for rows, C, relu in ((16, 256, True), (1000, 48, False), (333, 2048, True)):
            add(f"batchnorm-{rows}x{C}-{n}", TK, "test_batchnorm_train", (d, rows, C, relu), [bn])
        add(f"bn_relu_upsample_add-1x9x9x8-{n}", TK, "test_bn_relu_upsample_add_and_remask_backward", (d, (1, 9, 9, 8), 9, 9), [bn])
        add(f"bn_relu_upsample_add-2x10x14x32-{n}", TK, "test_bn_relu_upsample_add_and_remask_backward", (d, (2, 10, 14, 32), 4, 5),
            [bn, "iseg_resize_bilinear_bwd_workspace_bytes"])
        # ---- depthwise --------------------------------------------------------------------------------------------------------------
        add(f"dwconv-2x9x9x192-k7-{n}", TK, "test_dwconv_fwd_bwd", (d, (2, 9, 9, 192), 7, 1), ["iseg_dwconv2d_bwd_weight_workspace_bytes"])
        add(f"dwconv-1x20x11x64-k3-{n}", TK, "test_dwconv_fwd_bwd", (d, (1, 20, 11, 64), 3, 1), ["iseg_dwconv2d_bwd_weight_workspace_bytes"])
        add(f"dwconv_strided-1x15x9x16-k3s2-{n}", TK, "test_strided_depthwise_conv_matches_oracle", (d, (1, 15, 9, 16), 3, 2, 1),
            ["iseg_dwconv2d_strided_bwd_weight_workspace_bytes"])
        add(f"dwconv_strided-2x12x13x8-k5s2-{n}", TK, "test_strided_depthwise_conv_matches_oracle", (d, (2, 12, 13, 8), 5, 2, 1),
            ["iseg_dwconv2d_strided_bwd_weight_workspace_bytes"])
        # ---- bilinear resize --------------------------------------------------------------------------------------------------------
        for geo in ((7, 5, 13, 17, 8), (33, 31, 16, 16, 3), (1, 1, 4, 4, 2)):
            add(f"resize_bilinear-{'x'.join(map(str, geo))}-{n}", TK, "test_resize_bilinear_fwd_bwd", (d,) + geo,
                ["iseg_resize_bilinear_bwd_workspace_bytes"])
        add(f"upsample_ce-1x1x1x21-4x4-{n}", "tests.test_upsample_ce_gpu", "test_upsample_ce_matches_oracle_and_separate_kernels",
            (d, 1, 1, 1, 21, 4, 4), ["iseg_upsample_ce_workspace_bytes"])
        # ---- reductions -------------------------------------------------------------------------------------------------------------
        add(f"colsum_axpby_rowscale-{n}", TK, "test_colsum_broadcast_axpby_rowscale", (d,), ["iseg_colsum_workspace_bytes"])
        add(f"colsum_wide-5x8200-{n}", HERE, "_colsum_wide_case", (d, 5, 8200), ["iseg_colsum_wide_workspace_bytes"])
        add(f"mul_colsum-257x40-{n}", HERE, "_mul_colsum_case", (d, 257, 40), ["iseg_mul_colsum_workspace_bytes"])
        # ---- everything else that owns a workspace function -------------------------------------------------------------------------
        add(f"groupnorm-2x4x4x24-g1-{n}", MISC, "test_groupnorm", (d, (2, 4, 4, 24), 1), ["iseg_groupnorm_bwd_workspace_bytes"])
        add(f"rmsnorm-5x100-{n}", MISC, "test_rmsnorm", (d, 5, 100), ["iseg_rmsnorm_bwd_workspace_bytes"])
        add(f"grn-17x3x3x8-{n}", "tests.test_convnext_v2_gpu", "test_grn_forward_backward_match_oracle", (d, (17, 3, 3, 8)), ["iseg_grn_workspace_bytes"])
        add(f"pool_max-1x9x7x16-k3s2-{n}", MISC, "test_pool_same", (d, "max", (1, 9, 7, 16), 3, 2), ["iseg_pool2d_bwd_workspace_bytes"])
        add(f"pool_avg-1x5x5x8-k2s2-{n}", MISC, "test_pool_same", (d, "avg", (1, 5, 5, 8), 2, 2))
        add(f"replace_nan_or_inf-{n}", MISC, "test_replace_nan_or_inf", (d,))
        add(f"attention_plain-T37-{n}", "tests.test_attention_gpu", "test_attention_core_forward_backward", (d, "plain"))      # materialised route
        add(f"attention_swin-T49-{n}", "tests.test_attention_gpu", "test_attention_core_forward_backward", (d, "swin"))
        add(f"dcnv3_general_bwd-1x17x23x12-g4-{n}", "tests.test_dcnv3_gpu", "test_dcnv3_general_backward_is_bit_identical_and_right", (d, (1, 17, 23, 12), 4),
            ["iseg_dcnv3_bwd_workspace_bytes"])
        # (fp32: the bias gradient of the layer's GEMM is a column-sum pass of its own, the backward's first scratch user)
        add(f"dcnv2_layer-2x5x6x8-{n}", "tests.test_dcnv3_gpu", "test_dcnv2_layer_forward_and_gradients", (d, 2, 5, 6, 8, 16, True),
            ["iseg_dcnv2_sample_bwd_workspace_bytes"] if d == BF else ["iseg_colsum_workspace_bytes", "iseg_dcnv2_sample_bwd_workspace_bytes"])
        add(f"defattn-2x5x8x9-h3p3-{n}", "tests.test_deformable_mhsa_gpu", "test_deformable_attention_core_forward_backward", (d, ((2, 5, 8, 9), 3, 3, 2.0)),
            ["iseg_defattn_bwd_workspace_bytes"])
        add(f"relu_dwconv3_stats-s2-10x7-{n}", "tests.test_sepconv_fused_gpu", "test_stats_message", (d, 2, 10, 7), ["iseg_relu_dwconv3_stats_workspace_bytes"])
    # ---- GEMM, LDS-DMA pipeline (bf16) --------------------------------------------------------------------------------------------------
    add("gemm_dma-300x64x256", TK, "test_gemm_dma_pipeline_matches_oracle_and_register_staged_kernel", (300, 64, 256, 0))
    add("gemm_dma_ktail-300x64x72", TK, "test_gemm_dma_pipeline_k_tail", (300, 64, 72, 0))
    add("gemm_dma_strided_batch", TK, "test_gemm_dma_pipeline_strided_batch", ())
    # ---- depthwise on the matrix cores (bf16) -------------------------------------------------------------------------------------------
    add("dwconv7_mfma_fwd-1x5x7x32", "tests.test_dwconv_mfma_gpu", "test_dwconv7_mfma_forward_matches_oracle", (1, 5, 7, 32))
    add("dwconv7_mfma_dgrad-2x16x16x32", "tests.test_dwconv_mfma_gpu", "test_dwconv7_mfma_data_gradient_with_residual_matches_oracle", (2, 16, 16, 32))
    add("dwconv7_wgrad_mfma-9x9x32", "tests.test_dwconv_wgrad_mfma_gpu", "test_wgrad_mfma_matches_fp64", (9, 9, 32, False),
        ["iseg_dwconv2d_bwd_weight_workspace_bytes"])
    add("dwconv7_wgrad_mfma-16x16x32-acc", "tests.test_dwconv_wgrad_mfma_gpu", "test_wgrad_mfma_matches_fp64", (16, 16, 32, True),
        ["iseg_dwconv2d_bwd_weight_workspace_bytes"])
    # ---- implicit-GEMM convolution, all three passes (bf16) -----------------------------------------------------------------------------
    for i, c in enumerate((((2, 9, 7, 32), 3, 2, 1, 48, 1), ((2, 9, 9, 48), 3, 2, 2, 48, 3), ((1, 12, 12, 16), 2, 3, 1, 16, 1), ((1, 5, 5, 16), 3, 4, 1, 16, 1),
                           ((1, 16, 16, 768), 3, 1, 3, 256, 1), ((3, 17, 13, 64), 3, 2, 1, 128, 1))):
        add(f"conv_igemm-{'x'.join(map(str, c[0]))}-k{c[1]}s{c[2]}d{c[3]}-o{c[4]}g{c[5]}", "tests.test_conv_igemm_gpu", "test_conv_igemm_three_passes", c,
            ["iseg_conv2d_igemm_workspace_bytes"] if i == 4 else [])
    # ---- losses -------------------------------------------------------------------------------------------------------------------------
    add("resize_nearest_labels", TK, "test_resize_nearest_labels", ())
    for C in (3, 21, 150):
        add(f"softmax_ce-C{C}", TK, "test_softmax_ce_ignore", (C, 255, False), ["iseg_softmax_ce_workspace_bytes"])
        add(f"softmax_focal_ce-C{C}", TK, "test_softmax_focal_ce_ignore", (C, 255, False, 0.25, 2.0), ["iseg_softmax_ce_workspace_bytes"])
    add("mask_loss-C2-B1", "tests.test_mask_loss_gpu", "test_parity_classes_and_image_boundaries", (2, 1), ["iseg_mask_loss_workspace_bytes"])
    # ---- the rest of the workspace owners -----------------------------------------------------------------------------------------------
    add("flash_attention_inference-T130", "tests.test_attention_gpu", "test_inference_flash_attention_matches_materialised_route_and_oracle", (1, 5, 130))
    add("flash_attention_train-T65", "tests.test_range_edges_gpu", "test_flash_attention_with_a_late_dominant_key", (65, (0, 63, 64)),
        ["iseg_attention_bwd_workspace_bytes"])
    add("window_attention-T25", "tests.test_attention_gpu", "test_fused_window_attention_matches_materialised_route_and_oracle", (12, 4, 5, False),
        ["iseg_window_attention_bwd_workspace_bytes"])
    # (training mode: the batch statistics are the body's first scratch user; inference mode: the fused backward is)
    add("se_excite-1x7x9x32-se1", "tests.test_mbconv_fused_gpu", "test_fused_tail_fp32_matches_fp64", ((1, 7, 9, 32, 1), True),
        [bn, "iseg_se_excite_bwd_workspace_bytes"])
    add("se_excite_inference-1x7x9x32-se1", "tests.test_mbconv_fused_gpu", "test_fused_tail_fp32_matches_fp64", ((1, 7, 9, 32, 1), False),
        ["iseg_se_excite_bwd_workspace_bytes"], prelaunch=True)
    add("sepconv_unit-1x9x7x8to16", "tests.test_sepconv_fused_gpu", "test_fp32_against_fp64", ((1, 9, 7, 8, 16, 1, 1), True, MP),
        ["iseg_relu_dwconv3_stats_workspace_bytes", "iseg_bnfold_dwconv3_relu_bwd_workspace_bytes"])
    add("sepconv_unit_inference-bf16-1x9x7x8to16", "tests.test_sepconv_fused_gpu", "test_bf16_within_twice_composed_error", ((1, 9, 7, 8, 16, 1, 1), False, MP),
        ["iseg_bnfold_dwconv3_relu_bwd_workspace_bytes"])
    add("resblock_tail-bn0-s2-C32", "tests.test_resblock_fused_gpu", "test_tail_fp32_against_fp64", (True, 2, True, 32),
        [bn, "iseg_resblock_tail_workspace_bytes"])
    add("resblock_tail_inference-bn0-s2-C32", "tests.test_resblock_fused_gpu", "test_tail_fp32_against_fp64", (True, 2, False, 32),
        ["iseg_resblock_tail_workspace_bytes"])
    add("layerscale_grads", "tests.test_step_fusions_gpu", "test_layerscale_grads_from_split_k_slabs", (), ["iseg_layerscale_grads_workspace_bytes", gemm])
    add("convnext_mlp_wgrad-C96-M33", "tests.test_mlp_fused_gpu", "test_convnext_mlp_bwd_without_hidden_tensors_matches_oracle", (96, 33, 0, True),
        ["iseg_convnext_mlp_wgrad_workspace_bytes"])
    add("convnext_mlp_bwd_data_ln-C96-M1037", "tests.test_mlp_fused_gpu", "test_convnext_mlp_chain_through_the_layernorm_backward", (96, 1037),
        ["iseg_convnext_mlp_bwd_data_ln_workspace_bytes"])
    add("augment_means-contrast", "tests.test_augments_gpu", "test_photometric_class_matches_the_fused_standard_pipeline", ("contrast",),
        ["iseg_augment_means_workspace_bytes"])
    add("sod_metrics-37x53", "tests.test_sod_metrics_gpu", "test_parity_with_the_restatement", ("odd_37x53_saliency",), ["iseg_sod_metrics_workspace_bytes"])
    add("fmeasurev2-37x53", "tests.test_fmeasurev2_gpu", "test_parity_with_the_restatement", ("odd_37x53_saliency",), ["iseg_sod_fmv2_workspace_bytes"])
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
REFUSED = [c for c in CASES if c.refuses]      # the same body, every workspace 16 bytes short: its first scratch user has to refuse

# workspace function -> the entry points that take a workspace of that size, as _hip names them in a HipCallError
OWNERS = {
    "iseg_layernorm_bwd_workspace_bytes": ("iseg_layernorm_bwd", "iseg_layernorm_post_bwd", "iseg_layernorm_gather_bwd"),
    "iseg_bn_workspace_bytes": ("iseg_bn_stats", "iseg_bn_bwd_reduce", "iseg_bn_bwd_reduce_remask"),
    "iseg_resblock_tail_workspace_bytes": ("iseg_resblock_tail_bwd_reduce",),
    "iseg_dwconv2d_bwd_weight_workspace_bytes": ("iseg_dwconv2d_bwd_weight", "iseg_dwconv2d7_bwd_weight_mfma"),
    "iseg_conv2d_igemm_workspace_bytes": ("iseg_conv2d_igemm_fwd", "iseg_conv2d_igemm_fwd_kt", "iseg_conv2d_igemm_bwd_data", "iseg_conv2d_igemm_bwd_weight"),
    "iseg_augment_means_workspace_bytes": ("iseg_augment_channel_means",),
    "iseg_resize_bilinear_bwd_workspace_bytes": ("iseg_resize_bilinear_bwd", "iseg_resize_bilinear_ac_bwd"),
    "iseg_softmax_ce_workspace_bytes": ("iseg_softmax_ce_ignore", "iseg_softmax_focal_ce_ignore", "iseg_softmax_ce_confusion"),
    "iseg_grn_workspace_bytes": ("iseg_grn_fwd", "iseg_grn_bwd", "iseg_grn_bwd_folded"),
    "iseg_dcnv3_bwd_workspace_bytes": ("iseg_dcnv3_bwd", "iseg_dcnv3_bwd_ld"),
    "iseg_layerscale_grads_workspace_bytes": ("iseg_layerscale_grads", "iseg_layerscale_grads_slabs", "iseg_layerscale_grads_slabs_reduce"),
}


def owners(ws_function):
    """the entry points whose refusal counts for a workspace function (default: the function's own stem, iseg_x_workspace_bytes -> iseg_x)"""
    return OWNERS.get(ws_function, (ws_function[:-len("_workspace_bytes")],))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# two wrappers no test body calls directly: same style, the oracle is the fp64 sum of the stored values, the tolerance that of the colsum case of
# tests/test_kernels_gpu.py (fp32 accumulation over the rows of values of order one: 1e-4 of the largest sum for fp32 storage, 1e-3 for bf16)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _colsum_wide_case(cuda, dtype, rows, cols):
    """few rows, more than 8192 columns, not a multiple of the vector width's tile: kernels.colsum_wide and the route kernels.colsum takes to it"""
    from iseg_amd import kernels as k
    from tests import test_kernels_gpu as T

    x, xr = T.q(T.rnd((rows, cols), 1), dtype)
    out, _ = T.q(torch.zeros(cols, dtype=torch.float64), torch.float32)
    k.colsum_wide(x, out)
    T.close(out, xr.sum(0), torch.float32, "colsum_wide", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)
    k.colsum(x, cols, 0, 1, rows, cols, out, accumulate=True)
    T.close(out, 2 * xr.sum(0), torch.float32, "colsum -> colsum_wide, accumulated", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)


def _mul_colsum_case(cuda, dtype, rows, C):
    from iseg_amd import kernels as k
    from tests import test_kernels_gpu as T

    a, ar = T.q(T.rnd((rows, C), 1), dtype)
    b, br = T.q(T.rnd((rows, C), 2), dtype)
    out, _ = T.q(torch.full((C,), 0.5, dtype=torch.float64), torch.float32)
    k.mul_colsum(a, b, out, accumulate=True)
    T.close(out, (ar * br).sum(0) + 0.5, torch.float32, "mul_colsum (+)=", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)
    k.mul_colsum(a, b, out, accumulate=False)
    T.close(out, (ar * br).sum(0), torch.float32, "mul_colsum", f32_tol=1e-4 if dtype == torch.float32 else 1e-3)


# ---------------------------------------------------------------------------------------------------------------------------------------------
class _RecordingLib:
    """the loaded library with its iseg_*_workspace_bytes answers noted down: name -> largest answer"""

    def __init__(self, dll):
        self._dll, self.asked = dll, {}

    def __getattr__(self, name):
        fn = getattr(self._dll, name)
        if not name.endswith("_workspace_bytes"):
            return fn

        def ask(*a):
            n = fn(*a)
            self.asked[name] = max(self.asked.get(name, 0), int(n))
            return n

        return ask


@contextlib.contextmanager
def _recording():
    from iseg_amd import _hip

    dll = _hip.lib()
    rec = _RecordingLib(dll)
    _hip._lib = rec
    try:
        yield rec
    finally:
        _hip._lib = dll


@pytest.fixture(scope="module")
def arena(cuda):
    return GM.Arena(cuda)


def _body(case, cuda):
    fn = getattr(importlib.import_module(case.module), case.func)      # (imported before the scope opens: the scope re-routes the module's q)
    mp = pytest.MonkeyPatch()

    def run():
        from iseg_amd import nn

        try:
            fn(cuda, *[mp if a is MP else a for a in case.args])
        finally:
            mp.undo()
            nn.set_compute_dtype(torch.float32)

    return run


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_guarded(cuda, arena, case):
    run = _body(case, cuda)
    arena.reset()
    with _recording() as rec, GM.guarded(arena):
        run()
        arena.check()
        assert len(arena.records) > 0, "nothing was handed out of the arena: the body ran outside the guard"
    print("workspace functions asked:", rec.asked)
    for name in case.needs:
        assert rec.asked.get(name, 0) > 0, f"{case.id} is the ledger's case for {name}, which answered {rec.asked.get(name)} ({rec.asked})"


@pytest.mark.parametrize("case", REFUSED, ids=[c.id for c in REFUSED])
def test_launcher_refuses_a_workspace_16_bytes_short(cuda, arena, case):
    """the body's first scratch user is a launcher of case.refuses; it gets 16 bytes less than that function answered: that launcher (by name)
    returns ISEG_STATUS_WORKSPACE, and nothing was launched -- the short workspace and every buffer the refused call had allocated are still
    poison (prelaunch: every buffer from the short workspace on), and so are the bands"""
    from iseg_amd import _hip

    run = _body(case, cuda)
    arena.reset()
    with GM.guarded(arena, short_workspace=16) as scope:
        with pytest.raises(_hip.HipCallError, match=r"status -4\b") as e:
            run()
        refuser = str(e.value).split(" failed with status")[0]
        assert refuser in owners(case.refuses), f"{refuser} refused, not a launcher of {case.refuses}: {e.value}"
        arena.check()
        assert scope.refused_from is not None and scope.short_from is not None and scope.short_from >= scope.refused_from
        untouched, total = arena.untouched(role=None, since=scope.short_from if case.prelaunch else scope.refused_from)
        assert total >= 1 and untouched == total, f"{total - untouched} of the {total} buffers of the refused call were written: {arena.records[scope.refused_from:]}"
