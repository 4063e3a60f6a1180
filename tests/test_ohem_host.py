"""Online hard example mining on the host: the restatement tests/ohem_ref.py on hand-written answers, the two C ABI entries (declared, exported,
bound, no workspace function), the Python signatures of losses/ohem.py of the reference, and what is refused before any launch."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import ohem_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_all_zero_rows_give_thresh_itself():
    """nnz = 0: min_threshold = 0, threshold = max(0, thresh) = thresh; every probability is 0 < thresh, so every (zero) loss is 'kept'"""
    logits = np.arange(12, dtype=np.float64).reshape(4, 3)
    labels = np.array([255, 255, 3, -1])
    r = R.ohem(logits, labels, np.zeros(4, F32), 255, 2, 0.7, 100000)
    assert r["nnz"] == 0 and r["k"] is None and r["threshold"] == 0.7 and r["keep"].all() and not r["out"].any()
    assert not R.label_prob(logits, labels, 255).any()
    # ignore_label == 0 shifts: label 0 becomes the zero row, label 3 becomes class 2
    p = R.label_prob(logits, np.array([0, 1, 3, 4]), 0)
    assert p[0] == 0 and p[3] == 0 and p[1] > 0 and abs(p[2] - np.exp(2) / (1 + np.exp(1) + np.exp(2))) < 1e-15


def test_fewer_nonzero_than_min_kept_takes_the_smallest_nonzero_probability():
    """nnz - 1 < min_kept * N: k = nnz - 1, the descending sort's last non-zero entry; threshold = max(that, thresh)"""
    prob = np.array([0.9, 0.0, 0.2, 0.6, 0.0, 0.4], F32)
    loss = np.array([1, 2, 3, 4, 5, 6], F32)
    r = R.select_values(prob, loss, 100000 * 2, 0.1)
    assert r["nnz"] == 4 and r["k"] == 3 and r["threshold"] == F32(0.2)
    assert r["keep"].tolist() == [False, True, False, False, True, False] and r["out"].tolist() == [0, 2, 0, 0, 5, 0]
    r = R.select_values(prob, loss, 100000 * 2, 0.5)      # thresh above the smallest non-zero probability
    assert r["threshold"] == F32(0.5) and r["keep"].tolist() == [False, True, True, False, True, True]


def test_more_nonzero_than_min_kept_selects_above_thresh():
    """nnz - 1 > min_kept * N and the selected value above thresh: index k of the DESCENDING sort"""
    prob = np.array([0.9, 0.1, 0.8, 0.3, 0.7, 0.0, 0.5], F32)
    loss = np.arange(1, 8, dtype=F32)
    r = R.select_values(prob, loss, 1 * 2, 0.05)
    assert r["nnz"] == 6 and r["k"] == 2 and r["threshold"] == F32(0.7)
    assert r["keep"].tolist() == [False, True, False, True, False, True, True] and r["out"].tolist() == [0, 2, 0, 4, 0, 6, 7]


def test_ties_at_the_threshold_are_dropped():
    prob = np.array([0.5, 0.5, 0.5, 0.25, 0.75], F32)
    r = R.select_values(prob, np.ones(5, F32), 2, 0.1)
    assert r["threshold"] == F32(0.5) and r["keep"].tolist() == [False, False, False, True, False]
    loss = np.array([3, 1, 3, 2, 3, 0.5], F32)
    r = R.select_values(loss, loss, 2, None)      # sorted descending 3 3 3 2 1 0.5: index 2 is a 3, nothing is strictly above it
    assert r["threshold"] == 3 and not r["keep"].any()
    r = R.select_values(loss, loss, 3, None)
    assert r["threshold"] == 2 and r["keep"].tolist() == [True, False, True, False, True, False] and r["out"].tolist() == [3, 0, 3, 0, 3, 0]


def test_thresh_none_index_out_of_range():
    loss = np.ones(8, F32)
    assert R.select_values(loss, loss, 7, None)["k"] == 7
    with pytest.raises(ValueError):
        R.select_values(loss, loss, 8, None)
    with pytest.raises(ValueError):
        R.ohem(None, None, loss, 255, 4, None, 2)


def test_gpu_end_to_end_inputs_select_a_value_not_thresh():
    """the inputs of tests/test_ohem_gpu.py: with thresh = 0.05 and min_kept = 7 the threshold is the selected probability, and the restatement
    alone has one pixel within 1e-5 relative of it (the threshold's own); with the 0.7 / 100000 default k is nnz - 1"""
    from tests import test_ohem_gpu as T

    for shape in T.SHAPES:
        y, z = T.case(*shape)
        N = shape[0]
        r = R.ohem(z, y, np.zeros(y.size, F32), 255, N, 0.05, 7)
        assert r["nnz"] - 1 > 7 * N and r["k"] == 7 * N and r["threshold"] > 0.05
        assert int((np.abs(r["values"] - r["threshold"]) <= 1e-5 * r["threshold"]).sum()) == 1
        assert 0 < r["keep"].sum() < y.size
        r = R.ohem(z, y, np.zeros(y.size, F32), 255, N, 0.7, 100000)
        assert r["k"] == r["nnz"] - 1 and r["threshold"] == 0.7 and 0 < r["nnz"] < y.size


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------------
def _header():
    src = open(os.path.join(ROOT, "include", "iseg_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def hip():
    from iseg_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        from iseg_amd.build import build

        build(verbose=False)
    _hip.lib()
    return _hip


def test_entry_points_are_declared_exported_and_bound(hip):
    from iseg_amd import build, kernels

    dll = C.CDLL(hip.LIB_PATH)
    for name, nargs in (("iseg_ohem_label_prob", 7), ("iseg_ohem_select", 15)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
        assert hasattr(dll, name)
        res, args = hip.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    assert "ohem.hip" in build.SOURCES
    header = _header()
    assert int(re.search(r"#define\s+ISEG_OHEM_STATE_INTS\s+(\d+)", header).group(1)) == kernels.OHEM_STATE_INTS
    assert int(re.search(r"#define\s+ISEG_OHEM_PARTIAL_FLOATS\s+(\d+)", header).group(1)) == kernels.OHEM_PARTIAL_FLOATS


def test_no_workspace_function(hip):
    """the scratch is two typed blocks of fixed length: nothing to add to the workspace ledger"""
    names = re.findall(r"\b(iseg_[a-z0-9_]+)\s*\(", _header()) + list(hip.SIGNATURES)
    assert not [n for n in names if "ohem" in n and n.endswith("_workspace_bytes")]
    assert sorted(n for n in set(names) if "ohem" in n) == ["iseg_ohem_label_prob", "iseg_ohem_select"]


def test_wrappers_refuse_host_tensors(hip):
    from iseg_amd import kernels
    from iseg_amd.losses.ohem import get_ohem_fn, ohem_selector

    z, y, v = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int32), torch.rand(6)
    with pytest.raises(hip.HipCallError):
        kernels.ohem_label_prob(z, y, 255)
    with pytest.raises(hip.HipCallError):
        kernels.ohem_select(v, v, 2, 0.5)
    with pytest.raises(hip.HipCallError):
        kernels.ohem_select(v, v, 2, None)
    with pytest.raises(hip.HipCallError):
        ohem_selector(v, y, z, batch_size=1, thresh=0.5, min_kept=2)
    with pytest.raises(hip.HipCallError):
        get_ohem_fn(thresh=0.5)(y, z, v, 1)


def test_thresh_none_index_past_the_end_is_a_value_error_before_any_launch():
    """host tensors: a launch would have raised HipCallError first"""
    from iseg_amd import functional as F
    from iseg_amd import kernels
    from iseg_amd.losses.ohem import ohem_selector

    z, y, v = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int32), torch.rand(6)
    with pytest.raises(ValueError):
        ohem_selector(v, y, z, batch_size=2, thresh=None, min_kept=3)
    with pytest.raises(ValueError):
        F.ohem_softmax_ce_mean(z, y, 3, 255, 6, None)


def test_signatures_and_defaults_are_the_references():
    from iseg_amd.losses import ohem

    def spec(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert spec(ohem.ohem_selector) == [("loss", E), ("y_true", E), ("y_pred", E), ("batch_size", 4), ("thresh", None), ("min_kept", 100000)]
    assert spec(ohem.get_ohem_fn) == [("thresh", None), ("min_kept", 100000)]
    fn = ohem.get_ohem_fn()
    assert (fn.thresh, fn.min_kept) == (None, 100000)
    assert spec(fn) == [("y_true", E), ("y_pred", E), ("loss", E), ("batch_size", E)]
    fn = ohem.get_ohem_fn(thresh=0.7, min_kept=5)
    assert (fn.thresh, fn.min_kept) == (0.7, 5)


def test_seg_foundation_constructs_with_ohem_and_wires_the_main_output_only():
    from iseg_amd.core_model import SegFoundation
    from iseg_amd.losses.ohem import is_ohem_fn

    m = SegFoundation(num_class=5, use_ohem=True, ohem_thresh=0.6, num_aux_loss=1)
    assert m.use_ohem and m.ohem_thresh == 0.6
    losses = m.custom_losses(5, 255, 4)
    main, aux = losses["output_1"], losses["output_2"]
    assert callable(main.fused_mean) and main.fused_upsample_mean is None and main.confusion_spec == (5, 255)
    assert callable(aux.fused_mean) and callable(aux.fused_upsample_mean)
    plain = SegFoundation(num_class=5, num_aux_loss=1).custom_losses(5, 255, 4)
    assert callable(plain["output_1"].fused_upsample_mean)
    assert not is_ohem_fn(None) and not is_ohem_fn(lambda *a: None)


def test_other_post_compute_fns_are_called_as_before():
    """a post_compute_fn that is no OHEM selector still receives (None, y_pred, loss, batch) and switches the fused routes off"""
    from iseg_amd.losses.catecrossentropy_ignore_label import catecrossentropy_ignore_label_loss

    fn = catecrossentropy_ignore_label_loss(num_class=5, post_compute_fn=lambda yt, yp, lv, n: lv)
    assert fn.fused_mean is None and fn.fused_upsample_mean is None
    from iseg_amd.losses.ohem import get_ohem_fn

    assert catecrossentropy_ignore_label_loss(num_class=5, post_compute_fn=get_ohem_fn(0.7), reduction=True).fused_mean is None
