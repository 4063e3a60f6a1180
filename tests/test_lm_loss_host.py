"""The language-model head's cross-entropy without a GPU: the fp64 restatement (tests/lm_loss_ref.py) against closed forms, the argument checks
of F.lm_head_cross_entropy and GemmaCausalLM.compute_loss, their dry-run shapes, the chunk rule and the symbols of the built library."""
import math

import pytest
import torch

from tests import lm_loss_ref as R
from tests.test_gemma_gpu import CFG


# ---- the restatement against closed forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 5, 1000])
def test_uniform_logits_cost_log_v(V):
    x = torch.zeros(3, 4, dtype=torch.float64)
    E = torch.randn(V, 4, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    t = torch.tensor([0, V - 1, V // 2])
    out = R.forward(x, E, t)
    assert torch.allclose(out["loss"], torch.full((3,), math.log(V), dtype=torch.float64), rtol=0, atol=1e-12)
    assert out["argmax"].tolist() == [0, 0, 0]      # every logit ties: the first index
    assert out["match"].tolist() == [True, V == 1, V == 1]
    G, dX, dE = R.backward(x, E, t)
    assert torch.allclose(G.sum(dim=-1), torch.zeros(3, dtype=torch.float64), atol=1e-12)
    assert torch.allclose(dE, torch.zeros_like(dE))      # x = 0


def test_one_dominant_logit():
    """E = c I: row r of Z is c x_r; with x = e_k the target k costs log(1 + (V - 1) e^-c), any other c + that"""
    V, c = 6, 30.0
    E = c * torch.eye(V, dtype=torch.float64)
    x = torch.eye(V, dtype=torch.float64)[[2, 2]]
    out = R.forward(x, E, torch.tensor([2, 4]))
    tail = math.log1p((V - 1) * math.exp(-c))
    assert abs(out["loss"][0].item() - tail) < 1e-12 and abs(out["loss"][1].item() - (c + tail)) < 1e-9
    assert out["argmax"].tolist() == [2, 2] and out["match"].tolist() == [True, False]
    assert abs(out["sums"][1].item() - 1.0) < 1e-15 and abs(out["sums"][2].item() - 2.0) < 1e-15


def test_weight_zero_rows_and_targets_out_of_range():
    g = torch.Generator().manual_seed(2)
    x, E = torch.randn(5, 8, generator=g, dtype=torch.float64), torch.randn(7, 8, generator=g, dtype=torch.float64)
    t = torch.tensor([1, 7, -1, 3, 6])
    w = torch.tensor([1.0, 1.0, 1.0, 0.0, 2.0], dtype=torch.float64)
    out = R.forward(x, E, t, w, scale=0.5)
    assert out["loss"][1] == 0 and out["loss"][2] == 0 and out["loss"][3] == 0 and out["loss"][0] > 0 and out["loss"][4] > 0
    assert out["w"].tolist() == [1.0, 0.0, 0.0, 0.0, 2.0] and abs(out["sums"][2].item() - 3.0) < 1e-15
    assert not out["match"][1] and not out["match"][2]
    want = torch.nn.functional.cross_entropy(x @ E.T, t.clamp(0, 6), reduction="none")
    assert abs(out["loss"][4].item() - 0.5 * 2.0 * want[4].item()) < 1e-12
    G, dX, dE = R.backward(x, E, t, w, upstream=torch.tensor([1.0, 5.0, 5.0, 5.0, -3.0], dtype=torch.float64), scale=0.5)
    assert (G[1:4] == 0).all() and (dX[1:4] == 0).all()
    # against autograd on the same definition
    xa, Ea = x.clone().requires_grad_(True), E.clone().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(xa @ Ea.T, t.clamp(0, 6), reduction="none")
    (l * torch.tensor([0.5, 0, 0, 0, 0.5 * 2 * -3.0], dtype=torch.float64)).sum().backward()
    assert torch.allclose(dX, xa.grad, atol=1e-12) and torch.allclose(dE, Ea.grad, atol=1e-12)


def test_first_maximal_index_on_ties():
    Z = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 0.0, 0.0]], dtype=torch.float64)
    assert R.first_argmax(Z).tolist() == [1, 0, 0]
    assert R.accepted(Z, 1.0).tolist() == [[False, True, True, True], [True] * 4, [True, True, True, True]]


def test_keras_worked_example():
    """the fit(x, y, sample_weight) example of the reference's GemmaCausalLM docstring at the Gemma vocabulary, with logits that are all equal:
    every weighted token costs log 256000, "sum_over_batch_size" divides the sum by the 16 elements (not by the 12 weighted ones), and the
    accuracy is 0 of 12 -- the all-tie argmax is token 0, which is a target only where the weight is 0"""
    V = 256000
    y = torch.tensor([[214064, 603, 5271, 6044, 9581, 3, 0, 0]] * 2)
    sw = torch.tensor([[1, 1, 1, 1, 1, 1, 0, 0]] * 2, dtype=torch.float64)
    x = torch.zeros(2, 8, 2, dtype=torch.float64)
    E = torch.randn(V, 2, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    out = R.forward(x, E, y, sw)
    loss, acc = R.reduce(out["loss"], out["w"], out["match"])
    assert abs(loss.item() - 12 * math.log(V) / 16) < 1e-12 and acc.item() == 0.0
    assert abs(R.reduce(out["loss"], out["w"], out["match"], "sum")[0].item() - 12 * math.log(V)) < 1e-10
    assert tuple(R.reduce(out["loss"], out["w"], out["match"], "none")[0].shape) == (16,)
    # the weight-0 positions hold target 0 = the argmax: without the weights they would count
    assert out["match"].reshape(2, 8)[:, 6:].all() and not out["match"].reshape(2, 8)[:, :6].any()


# ---- argument checks ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fp32_cpu():
    from iseg_amd import nn

    nn.set_compute_dtype(torch.float32)
    nn.set_device("cpu")
    yield nn
    nn.set_device(None)


def test_function_refuses_bad_arguments(fp32_cpu):
    from iseg_amd import functional as F

    h, E, t = torch.zeros(2, 3, 8), torch.nn.Parameter(torch.zeros(11, 8)), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(TypeError, match="compute dtype"):
        F.lm_head_cross_entropy(h.to(torch.bfloat16), E, t)
    with pytest.raises(ValueError, match="hidden is"):
        F.lm_head_cross_entropy(h, torch.nn.Parameter(torch.zeros(11, 9)), t)
    with pytest.raises(ValueError, match="target_ids has the shape"):
        F.lm_head_cross_entropy(h, E, t[:, :2])
    with pytest.raises(ValueError, match="int32 or int64"):
        F.lm_head_cross_entropy(h, E, t.float())
    with pytest.raises(ValueError, match="sample_weight has the shape"):
        F.lm_head_cross_entropy(h, E, t, torch.ones(2, 2))
    with pytest.raises(ValueError, match="floating-point"):
        F.lm_head_cross_entropy(h, E, t, torch.ones(2, 3, dtype=torch.int32))
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="chunk is"):
            F.lm_head_cross_entropy(h, E, t, chunk=bad)
    with pytest.raises(ValueError, match="finite"):
        F.lm_head_cross_entropy(h, E, t, upstream_scale=float("inf"))
    with pytest.raises(RuntimeError, match="hidden and table only"):
        F.lm_head_cross_entropy(h, E, t, torch.ones(2, 3, requires_grad=True))


def test_mixed_precision_without_a_shadow_is_refused():
    """bf16 compute and a table that has no bf16 copy: refused as the neighbouring functions refuse it, nothing runs"""
    from iseg_amd import functional as F
    from iseg_amd import nn

    nn.set_compute_dtype(torch.bfloat16)
    try:
        with pytest.raises(RuntimeError, match="no bf16 shadow"):
            F.lm_head_cross_entropy(torch.zeros(2, 8, dtype=torch.bfloat16), torch.nn.Parameter(torch.zeros(11, 8)), torch.zeros(2, dtype=torch.int64))
    finally:
        nn.set_compute_dtype(torch.float32)


def test_function_dry_run_shapes(fp32_cpu):
    from iseg_amd import functional as F

    h, E, t = torch.zeros(2, 3, 8), torch.nn.Parameter(torch.zeros(11, 8)), torch.zeros(2, 3, dtype=torch.int64)
    with fp32_cpu.dry_run_scope():
        loss = F.lm_head_cross_entropy(h, E, t)
        both = F.lm_head_cross_entropy(h, E, t, torch.ones(2, 3), chunk=4, with_accuracy=True)
    assert tuple(loss.shape) == (2, 3) and loss.dtype == torch.float32
    assert tuple(both[0].shape) == (2, 3) and tuple(both[1].shape) == (2, 3) and both[1].dtype == torch.int32


def _cpu_model():
    from iseg_amd.nlp.gemma import GemmaBackbone, GemmaCausalLM

    return GemmaCausalLM(GemmaBackbone(**CFG))


def test_compute_loss_dry_run_shapes_and_refusals(fp32_cpu, monkeypatch):
    model = _cpu_model()
    ids = torch.zeros(2, 9, dtype=torch.int64)
    inputs = {"token_ids": ids, "padding_mask": torch.ones(2, 9, dtype=torch.int32)}
    for fused in ("1", "0"):
        monkeypatch.setenv("ISEG_LMHEAD_FUSED", fused)
        with fp32_cpu.dry_run_scope():
            assert tuple(model.compute_loss(inputs, ids).shape) == ()
            assert tuple(model.compute_loss(inputs, ids, reduction="sum").shape) == ()
            loss, metrics = model.compute_loss(inputs, ids, torch.ones(2, 9), reduction="none", with_metrics=True)
            assert tuple(loss.shape) == (2, 9) and loss.dtype == torch.float32
            assert list(metrics) == ["sparse_categorical_accuracy"] and tuple(metrics["sparse_categorical_accuracy"].shape) == ()
            with pytest.raises(ValueError, match="reduction is"):
                model.compute_loss(inputs, ids, reduction="mean")
            with pytest.raises(ValueError, match="y has the shape"):
                model.compute_loss(inputs, ids[:, :8])
            with pytest.raises(ValueError, match="sample_weight has the shape"):
                model.compute_loss(inputs, ids, torch.ones(2, 8))


# ---- the chunk rule and the library ---------------------------------------------------------------------------------------------------------------
def test_chunk_rule_stays_inside_the_vocabulary():
    """chunk = 0: a width in [1, V] for every V from 1 to 2^20, at one row and at many; the chunks cover the vocabulary once, never 0 chunks"""
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    rule = _hip.lib().iseg_lm_head_ce_chunk_default
    for M in (1, 8192):
        assert all(1 <= rule(M, V) <= V for V in range(1, (1 << 20) + 1)), M
    assert rule(8192, 0) == 0 and rule(8192, -3) == 0
    for V in (1, 2, 5, 255, 256, 8191, 8192, 8193, 256000, 1 << 20):
        c = K.lm_head_ce_chunk_default(8192, V)
        chunks = K.lm_head_ce_chunks(V, c)
        assert len(chunks) >= 1 and chunks[0][0] == 0 and sum(w for _, w in chunks) == V and all(1 <= w <= c for _, w in chunks)
        assert all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert K.lm_head_ce_chunks(1000, 256) == [(0, 256), (256, 256), (512, 256), (768, 232)]
    assert K.lm_head_ce_pitch(232) == 232 and K.lm_head_ce_pitch(5) == 8 and K.lm_head_ce_pitch(1) == 8


def test_abi_symbols_exist_in_the_built_library():
    from iseg_amd import _hip

    L = _hip.lib()
    for name in ("iseg_lm_head_ce_chunk_default", "iseg_lm_head_ce_scratch_bytes", "iseg_lm_head_ce_chunk_fwd", "iseg_lm_head_ce_target_logit",
                 "iseg_lm_head_ce_finalise",
                 "iseg_lm_head_ce_chunk_bwd"):
        assert name in _hip.SIGNATURES and getattr(L, name) is not None, name
    assert L.iseg_lm_head_ce_scratch_bytes(0) == 0 and L.iseg_lm_head_ce_scratch_bytes(1) == 12
    assert L.iseg_lm_head_ce_scratch_bytes(256) == 12 and L.iseg_lm_head_ce_scratch_bytes(257) == 24


def test_launchers_refuse_bad_arguments_without_a_gpu():
    """the argument checks come before any launch: null pointers, an empty chunk, a short pitch and a short scratch buffer are refused on the host"""
    from iseg_amd import _hip

    L = _hip.lib()
    p = 4096      # a non-null placeholder: a refused call dereferences nothing
    assert L.iseg_lm_head_ce_chunk_fwd(None, 8, p, p, p, p, p, 4, 0, 8, None) == -1
    assert L.iseg_lm_head_ce_chunk_fwd(p, 8, p, p, p, p, p, 4, 0, 0, None) == -1
    assert L.iseg_lm_head_ce_chunk_fwd(p, 7, p, p, p, p, p, 4, 0, 8, None) == -1
    assert L.iseg_lm_head_ce_chunk_fwd(p, 8, p, p, p, p, p, 4, (1 << 31) - 8, 8, None) == -1
    assert L.iseg_lm_head_ce_target_logit(p, 7, p, 8, p, p, 4, 16, 8, 0, None) == -1      # short pitch of x
    assert L.iseg_lm_head_ce_target_logit(p, 8, p, 8, p, None, 4, 16, 8, 0, None) == -1
    assert L.iseg_lm_head_ce_target_logit(p, 8, p, 8, p, p, 4, 16, 8, 5, None) == -1      # dtype
    assert L.iseg_lm_head_ce_finalise(p, p, p, p, p, None, p, p, p, p, p, 11, 4, 8, 1.0, None) == -4
    assert L.iseg_lm_head_ce_finalise(p, p, p, p, p, None, p, p, p, p, None, 0, 4, 8, 1.0, None) == -4
    assert L.iseg_lm_head_ce_chunk_bwd(p, 8, p, p, p, None, None, 1.0, p, 8, 4, 8, 4, 8, 0, None) == -1      # the chunk leaves the vocabulary
    assert L.iseg_lm_head_ce_chunk_bwd(p, 8, p, p, p, None, None, 1.0, p, 7, 4, 16, 0, 8, 1, None) == -1     # short pitch of G
    assert L.iseg_lm_head_ce_chunk_bwd(p, 8, p, p, p, None, None, 1.0, p, 8, 4, 16, 0, 8, 7, None) == -1     # dtype
