"""The guard-band helper (tests/guarded_memory.py) is not vacuous, and every workspace function of the C ABI is placed: covered by a guarded
GPU test or exempted with a reason.  CPU only."""
import os
import re

import pytest
import torch

from tests import guarded_memory as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 4 << 20      # a CPU arena: 1 MiB margins and 64 KiB bands as on the device, 2 MiB to hand out


@pytest.fixture()
def arena():
    return GM.Arena("cpu", SMALL)


def _violation(arena):
    with pytest.raises(GM.GuardViolation) as e:
        arena.check()
    return e.value


def _view_past(arena, t, first_elem, n):
    """n elements of t's dtype starting first_elem elements from t's first (negative: in front of it) -- what a kernel with a wrong bound addresses"""
    item = t.element_size()
    a = arena.offset_of(t) + first_elem * item
    return arena.buf[a:a + n * item].view(t.dtype)


def test_untouched_arena_and_writes_inside_a_view_pass(arena):
    arena.check()
    x = arena.alloc((7, 5), torch.float32, "output", name="x")
    y = arena.alloc((3,), torch.bfloat16, "operand", name="y")
    arena.check()
    x.fill_(1.5)
    y.copy_(torch.tensor([1.0, 2.0, 3.0]))
    x[6, 4] = -2.0      # its last element
    x[0, 0] = 3.0       # and its first
    arena.check()
    assert x.sum().item() == 1.5 * 33 + 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32, torch.uint8])
def test_one_element_past_the_end_is_reported(arena, dtype):
    arena.alloc((5,), torch.float32, "operand", name="left")
    x = arena.alloc((7, 5), dtype, "output", name="x")
    arena.alloc((9,), torch.float32, "workspace", name="right")
    _view_past(arena, x, x.numel(), 1).fill_(0)
    v = _violation(arena)
    assert v.record.name == "x" and v.record.role == "output" and v.record.shape == (7, 5) and v.record.dtype == dtype
    assert v.side == "after" and v.distance == 0
    assert v.offset == arena.offset_of(x) + x.numel() * x.element_size()
    assert "'x'" in str(v) and "output" in str(v) and "(7, 5)" in str(v) and "0 bytes past the end" in str(v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_element_before_the_start_is_reported(arena, dtype):
    arena.alloc((5,), torch.float32, "operand", name="left")
    x = arena.alloc((4, 3), dtype, "workspace", name="ws")
    _view_past(arena, x, -1, 1).fill_(0)
    v = _violation(arena)
    assert v.record.name == "ws" and v.record.role == "workspace"
    assert v.side == "before" and v.distance == x.element_size()
    assert v.offset == arena.offset_of(x) - x.element_size()
    assert f"{x.element_size()} bytes before the start" in str(v)


def test_single_byte_in_distant_free_space_is_reported(arena):
    x = arena.alloc((16,), torch.float32, "output", name="x")
    far = arena.offset_of(x) + 16 * 4 + 700_001
    arena.buf[far] = 0xFE
    v = _violation(arena)
    assert v.offset == far and v.record.name == "x" and v.side == "after" and v.distance == 700_001
    assert "0xfe" in str(v) and "(1 bytes changed in all)" in str(v)
    arena.buf[far] = GM.POISON
    arena.check()
    arena.buf[3] = 0        # inside the margin nobody is given
    assert _violation(arena).offset == 3


def test_a_changed_byte_with_nothing_handed_out_is_reported(arena):
    arena.buf[SMALL - 1] = 0
    assert _violation(arena).record is None


def test_offsets_bands_and_margins(arena):
    ts = [arena.alloc(s, d, "operand") for s, d in (((3,), torch.float32), ((1000, 7), torch.bfloat16), ((1,), torch.uint8), ((513,), torch.int32))]
    for t in ts:
        assert t.data_ptr() % 512 == 16 and t.is_contiguous()
        assert bool((t.view(-1).view(torch.uint8) == GM.POISON).all())
    recs = arena.records
    assert recs[0].start >= GM.MARGIN + GM.BAND
    for a, b in zip(recs, recs[1:]):
        assert b.start - a.end >= GM.BAND
    assert arena.alloc((8,), torch.float32, "operand", align=512).data_ptr() % 512 == 0
    assert torch.isnan(ts[0]).all() and torch.isnan(ts[1].float()).all() and (ts[3] == -1).all()
    with pytest.raises(MemoryError):
        arena.alloc((SMALL,), torch.uint8, "output")
    big = arena.alloc((SMALL - 2 * GM.MARGIN - 8 * GM.BAND,), torch.uint8, "output")      # what is left, and still a margin behind it
    assert arena.offset_of(big) + big.numel() <= SMALL - GM.MARGIN - GM.BAND
    arena.reset()
    assert arena.records == [] and bool((arena.buf == GM.POISON).all())


def test_patched_workspace_and_allocations():
    from iseg_amd import _hip, kernels

    arena = GM.Arena("cpu", SMALL)
    real_ws, real_torch = kernels.workspace, kernels.torch
    cpu = torch.device("cpu")
    with GM.guarded(arena, kernels=kernels):
        assert kernels.workspace(0, cpu) == (None, 0) and kernels.workspace(-8, cpu) == (None, 0)
        ws, n = kernels.workspace(1000, cpu)
        assert n == 1000 and ws.numel() == 1000 and ws.dtype == torch.uint8 and ws.data_ptr() % 512 == 16
        ws.zero_()
        ws2, n2 = kernels.workspace(1000, cpu)      # the next launcher finds poison, not the last one's partials
        assert n2 == 1000 and ws2.data_ptr() == ws.data_ptr() and bool((ws2 == GM.POISON).all())
        ws3, n3 = kernels.workspace(1016, cpu)
        assert n3 == 1016 and ws3.numel() == 1016 and ws3.data_ptr() != ws.data_ptr()
        T = kernels.torch
        e = T.empty((3, 5), dtype=torch.float32, device=cpu)
        e2 = T.empty(4, 2, dtype=torch.bfloat16, device="cpu")
        z = T.zeros((6,), dtype=torch.float32, device=cpu)
        f = T.full((2, 2), 0.5, dtype=torch.float32, device=cpu)
        o = T.ones_like(e)
        el = T.empty_like(e2)
        zl = T.zeros_like(e, dtype=torch.int32)
        perm = torch.zeros(4, 6).t()
        pl = T.empty_like(perm)
        for t in (e, e2, z, f, o, el, zl, pl):
            assert 0 <= arena.offset_of(t) < SMALL and t.data_ptr() % 512 == 16
        assert torch.isnan(e).all() and torch.isnan(e2.float()).all() and torch.isnan(el.float()).all() and e2.shape == (4, 2)
        assert (z == 0).all() and (f == 0.5).all() and (o == 1).all() and (zl == 0).all() and zl.dtype == torch.int32
        assert pl.shape == perm.shape and pl.stride() == perm.stride()
        assert T.float32 is torch.float32 and T.Tensor is torch.Tensor      # everything else is torch's own
        assert T.empty(0, dtype=torch.float32, device=cpu).numel() == 0
        roles = [r.role for r in arena.records]
        assert roles.count("workspace") == 2 and roles.count("output") == 8
        arena.check()
        assert arena.untouched("output") == (4, 8)      # e, e2, el, pl
    assert kernels.workspace is real_ws and kernels.torch is real_torch
    real_fwd = kernels.layernorm_fwd
    with GM.guarded(arena, short_workspace=16, kernels=kernels) as scope:
        ws, n = kernels.workspace(1000, cpu)
        assert n == 984 and ws.numel() == 984
        assert kernels.workspace(16, cpu) == (None, 0)
        before = len(arena.records)
        with pytest.raises(_hip.HipCallError):      # (no CPU path: the call raises, and the scope notes where the raising call began)
            kernels.layernorm_fwd(torch.zeros(8, 8), torch.ones(8), torch.zeros(8), 1e-6)
        assert scope.refused_from == before
    assert kernels.workspace is real_ws and kernels.layernorm_fwd is real_fwd


def test_patched_operand_helper_puts_q_into_the_arena():
    from iseg_amd import kernels
    from tests import test_kernels_gpu as TK

    arena = GM.Arena("cpu", SMALL)
    real_q = TK.q
    x = torch.arange(12, dtype=torch.float64).reshape(3, 4) / 3
    with GM.guarded(arena, kernels=kernels):
        d, r = TK.q(x, torch.bfloat16)
        assert d.dtype == torch.bfloat16 and r.dtype == torch.float64 and torch.equal(d.double(), r) and torch.equal(r, x.to(torch.bfloat16).double())
        assert arena.records[-1].role == "operand" and d.data_ptr() % 512 == 16
        _view_past(arena, d, d.numel(), 1).fill_(0)
        assert _violation(arena).record.role == "operand"
    assert TK.q is real_q


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the coverage ledger: every iseg_*_workspace_bytes the header declares is placed
# ---------------------------------------------------------------------------------------------------------------------------------------------
GUARDED = "tests.test_guarded_memory_gpu::test_guarded"

# workspace function -> the case of tests/test_guarded_memory_gpu.py that runs its launcher inside the guard with a workspace of exactly that size
# (the case fails unless the function was asked and answered more than zero) and in which that launcher is the body's first scratch user: run
# 16 bytes short in test_launcher_refuses_a_workspace_16_bytes_short, it is the launcher that has to refuse, by name
COVERED = {
    "iseg_gemm_workspace_bytes": "gemm_wgrad_split3-1030x21x256-bf16",
    "iseg_layernorm_bwd_workspace_bytes": "layernorm_post-520x112x4-ttt-bf16",
    "iseg_bn_workspace_bytes": "batchnorm-333x2048-bf16",
    "iseg_dwconv2d_bwd_weight_workspace_bytes": "dwconv-2x9x9x192-k7-bf16",
    "iseg_dwconv2d_strided_bwd_weight_workspace_bytes": "dwconv_strided-2x12x13x8-k5s2-f32",
    "iseg_conv2d_igemm_workspace_bytes": "conv_igemm-1x16x16x768-k3s1d3-o256g1",
    "iseg_resize_bilinear_bwd_workspace_bytes": "resize_bilinear-7x5x13x17x8-f32",
    "iseg_upsample_ce_workspace_bytes": "upsample_ce-1x1x1x21-4x4-f32",
    "iseg_softmax_ce_workspace_bytes": "softmax_ce-C21",
    "iseg_mask_loss_workspace_bytes": "mask_loss-C2-B1",
    "iseg_colsum_workspace_bytes": "colsum_axpby_rowscale-bf16",
    "iseg_colsum_wide_workspace_bytes": "colsum_wide-5x8200-bf16",
    "iseg_mul_colsum_workspace_bytes": "mul_colsum-257x40-f32",
    "iseg_groupnorm_bwd_workspace_bytes": "groupnorm-2x4x4x24-g1-f32",
    "iseg_rmsnorm_bwd_workspace_bytes": "rmsnorm-5x100-bf16",
    "iseg_grn_workspace_bytes": "grn-17x3x3x8-bf16",
    "iseg_pool2d_bwd_workspace_bytes": "pool_max-1x9x7x16-k3s2-bf16",
    "iseg_attention_bwd_workspace_bytes": "flash_attention_train-T65",
    "iseg_window_attention_bwd_workspace_bytes": "window_attention-T25",
    "iseg_dcnv3_bwd_workspace_bytes": "dcnv3_general_bwd-1x17x23x12-g4-f32",
    "iseg_dcnv2_sample_bwd_workspace_bytes": "dcnv2_layer-2x5x6x8-bf16",
    "iseg_defattn_bwd_workspace_bytes": "defattn-2x5x8x9-h3p3-bf16",
    "iseg_se_excite_bwd_workspace_bytes": "se_excite_inference-1x7x9x32-se1",
    "iseg_relu_dwconv3_stats_workspace_bytes": "relu_dwconv3_stats-s2-10x7-bf16",
    "iseg_bnfold_dwconv3_relu_bwd_workspace_bytes": "sepconv_unit_inference-bf16-1x9x7x8to16",
    "iseg_resblock_tail_workspace_bytes": "resblock_tail_inference-bn0-s2-C32",
    "iseg_layerscale_grads_workspace_bytes": "layerscale_grads",
    "iseg_convnext_mlp_wgrad_workspace_bytes": "convnext_mlp_wgrad-C96-M33",
    "iseg_convnext_mlp_bwd_data_ln_workspace_bytes": "convnext_mlp_bwd_data_ln-C96-M1037",
    "iseg_augment_means_workspace_bytes": "augment_means-contrast",
    "iseg_sod_metrics_workspace_bytes": "sod_metrics-37x53",
    "iseg_sod_fmv2_workspace_bytes": "fmeasurev2-37x53",
}

# workspace function -> why no guarded case runs it (one sentence each; at most MAX_EXEMPT)
NOT_COVERED = {}
MAX_EXEMPT = 6


def _declared_workspace_functions():
    src = open(os.path.join(ROOT, "include", "iseg_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(n for n in set(re.findall(r"\b(?:int|size_t)\s+(iseg_[a-z0-9_]+)\s*\(", src)) if n.endswith("_workspace_bytes"))


def test_every_declared_workspace_function_is_placed():
    declared = _declared_workspace_functions()
    assert len(declared) >= 30 and "iseg_gemm_workspace_bytes" in declared
    assert len(NOT_COVERED) <= MAX_EXEMPT
    assert not set(COVERED) & set(NOT_COVERED)
    for name in declared:
        assert name in COVERED or name in NOT_COVERED, f"{name} is declared in iseg_hip.h: give it a guarded case (COVERED) or a reason (NOT_COVERED)"
    for name in list(COVERED) + list(NOT_COVERED):
        assert name in declared, f"{name} is in the ledger but iseg_hip.h no longer declares it"
    for name, why in NOT_COVERED.items():
        assert isinstance(why, str) and len(why.split()) >= 5 and why.strip().endswith("."), f"{name}: a one-sentence reason, please"


def test_covered_entries_name_guarded_cases_that_demand_the_function():
    from tests import test_guarded_memory_gpu as G

    refused = {c.id for c in G.REFUSED}
    for name, cid in COVERED.items():
        case = G.BY_ID.get(cid)
        assert case is not None, f"{name}: no case {GUARDED}[{cid}]"
        assert name in case.needs, f"{GUARDED}[{cid}] does not demand a non-zero {name}"
        assert cid in refused and case.refuses == name, f"{cid} is not run short with a launcher of {name} as its first scratch user"
        assert all(o.startswith("iseg_") and not o.endswith("_workspace_bytes") for o in G.owners(name))
