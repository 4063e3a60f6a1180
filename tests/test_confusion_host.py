"""Confusion matrices on the host: the numpy restatement tests/confusion_ref.py on hand-written answers, the shape checks that come before
any launch, get_per_class_miou's batch / axis / dtype keywords on CPU tensors, the fixed-point exponent and its error bound, the C ABI of
csrc/confusion.hip (declared, exported, bound, no workspace function) and what the launcher refuses before it touches the device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import confusion_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"iseg_confusion_supported": 2, "iseg_confusion_absmax_f32": 4, "iseg_confusion_batched": 14}


# ---- the restatement and the reference's own example ---------------------------------------------------------------------------------------
def test_reference_docstring_example():
    """tf.math.confusion_matrix([1, 2, 4], [2, 2, 4]) of metrics/confusion_matrix.py:80-86"""
    want = np.zeros((5, 5), np.int32)
    want[1, 2] = want[2, 2] = want[4, 4] = 1
    got = R.confusion_matrix([1, 2, 4], [2, 2, 4])
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(R.batch_confusion_matrix([[1, 2, 4]], [[2, 2, 4]])[0], want)
    cm, counters = R.kernel_counts([[1, 2, 4]], [[2, 2, 4]], 5)
    assert np.array_equal(cm[0], want) and not counters.any()
    w = R.confusion_matrix([1, 2, 4], [2, 2, 4], weights=[0.5, 2.0, 3.0], dtype=np.float32)
    assert w[1, 2] == 0.5 and w[2, 2] == 2.0 and w[4, 4] == 3.0 and w.sum() == 5.5
    for bad, msg in ((([-1, 2], [0, 0], None), 0), (([1, 2], [0, -3], None), 1), (([1, 5], [0, 0], 5), 2), (([1, 2], [0, 7], 5), 3)):
        with pytest.raises(ValueError, match=re.escape(R.MESSAGES[msg])):
            R.confusion_matrix(*bad)


def test_restated_kernel_rules():
    """ignore is looked at first; every failed check bumps its counter; a rounded weight is counted and still added"""
    lab = np.array([[0, 1, 255, 255, -2, 3, 1, 1]])
    prd = np.array([[0, 1, -5, 3, 0, 1, -1, 2]])
    cm, c = R.kernel_counts(lab, prd, 3, ignore_label=255)
    assert c.tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and cm.sum() == 3 and cm[0, 0, 0] == cm[0, 1, 1] == cm[0, 1, 2] == 1
    w = np.array([[0.5, 1.5, 2.5, np.nan, np.inf, 1.0, 2.0 ** 39, 0.25]], np.float32)
    cm, c = R.kernel_counts(np.zeros((1, 8), int), np.zeros((1, 8), int), 1, w, 0)
    assert c.tolist() == [0, 0, 0, 0, 3, 4, 0, 0] and cm[0, 0, 0] == 0 + 2 + 2 + 1 + 0      # half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2


def test_remove_squeezable_dimensions():
    from iseg_amd.metrics.confusion_matrix import remove_squeezable_dimensions

    a, b = torch.zeros(4, 3), torch.zeros(4, 3, 1)
    for fn, mk in ((remove_squeezable_dimensions, lambda t: t), (R.remove_squeezable_dimensions, lambda t: t.numpy())):
        l, p = fn(mk(a), mk(b))
        assert tuple(l.shape) == (4, 3) and tuple(p.shape) == (4, 3)
        l, p = fn(mk(b), mk(a))
        assert tuple(l.shape) == (4, 3) and tuple(p.shape) == (4, 3)
        l, p = fn(mk(a), mk(a))
        assert tuple(l.shape) == (4, 3) and tuple(p.shape) == (4, 3)
        l, p = fn(mk(a), mk(torch.zeros(4, 3, 2)))      # last dimension is not 1: nothing is squeezed
        assert tuple(l.shape) == (4, 3) and tuple(p.shape) == (4, 3, 2)
        l, p = fn(mk(a), mk(b), 1)      # expected_rank_diff = 1: already as expected
        assert tuple(l.shape) == (4, 3) and tuple(p.shape) == (4, 3, 1)
        l, p = fn(mk(torch.zeros(4, 1)), mk(torch.zeros(4, 1)), 1)      # ranks equal where one more was expected: the labels lose their 1
        assert tuple(l.shape) == (4,) and tuple(p.shape) == (4, 1)
        l, p = fn(mk(torch.zeros(4)), mk(torch.zeros(4, 3, 1)), 1)      # two more: the predictions lose theirs
        assert tuple(l.shape) == (4,) and tuple(p.shape) == (4, 3)


def test_signatures_and_defaults_are_the_references():
    from iseg_amd.metrics import confusion_matrix as M
    from iseg_amd.metrics import mean_iou as I
    from iseg_amd.metrics import seg_metric_wrapper as S

    def spec(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert spec(M.remove_squeezable_dimensions) == [("labels", E), ("predictions", E), ("expected_rank_diff", 0), ("name", None)]
    cm_spec = [("labels", E), ("predictions", E), ("num_classes", None), ("weights", None), ("dtype", torch.int32), ("name", None)]
    assert spec(M.confusion_matrix) == cm_spec and spec(M.batch_confusion_matrix) == cm_spec
    cls_spec = [("y_true", E), ("y_pred", E), ("num_class", 21), ("sample_weight", None), ("dtype", torch.float32)]
    assert spec(I.get_class_confusion_matrix) == cls_spec and spec(I.get_batch_class_confusion_matrix) == cls_spec
    assert spec(I.get_per_class_miou) == [("cm", E), ("dtype", None), ("row_axis", -2), ("col_axis", -1)]
    assert spec(I.MeanIOU.update_state) == [("self", E), ("y_true", E), ("y_pred", E), ("sample_weight", None)]
    assert spec(S.process_seg_metric_inputs) == [("y_true", E), ("y_pred", E), ("num_class", 21), ("ignore_label", 255), ("use_class_prob_as_pred", True),
                                                 ("flatten_outputs", True), ("set_ignore_label_to_zero", True)]


def test_mismatched_shapes_raise_value_error_before_the_library_is_touched(monkeypatch):
    """CPU tensors: a launch would have raised HipCallError; and the library is made unloadable for the duration"""
    from iseg_amd import _hip
    from iseg_amd.metrics import confusion_matrix as M

    monkeypatch.setattr(_hip, "_lib", None)
    monkeypatch.setattr(_hip, "LIB_PATH", "/nonexistent/libiseg_hip.so")
    y = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError):
        M.confusion_matrix(y, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError):
        M.confusion_matrix(y.reshape(2, 3), y.reshape(2, 3))      # 1-D only
    with pytest.raises(ValueError):
        M.confusion_matrix(y, y, 3, weights=torch.ones(5))
    with pytest.raises(ValueError):
        M.batch_confusion_matrix(y.reshape(2, 3), y.reshape(3, 2))
    with pytest.raises(ValueError):
        M.batch_confusion_matrix(torch.tensor(1), torch.tensor(1))      # rank 0
    with pytest.raises(ValueError):
        M.batch_confusion_matrix(y.reshape(2, 3), y.reshape(2, 3), 3, weights=torch.ones(2, 2))
    with pytest.raises(_hip.HipCallError):      # well-formed host tensors: there is no CPU path
        M.confusion_matrix(y, y, 3)


# ---- get_per_class_miou ------------------------------------------------------------------------------------------------------------------
def _old_get_per_class_miou(cm):
    """the function as it stood before the keywords were added"""
    cm = cm.to(torch.float64)
    sum_over_row = cm.sum(-2)
    sum_over_col = cm.sum(-1)
    tp = torch.diagonal(cm, dim1=-2, dim2=-1)
    denom = sum_over_row + sum_over_col - tp
    num_valid = (denom != 0).to(torch.float64).sum(-1)
    iou = torch.where(denom != 0, tp / torch.where(denom != 0, denom, torch.ones_like(denom)), torch.zeros_like(denom))
    return iou, num_valid


def test_get_per_class_miou_batched_axes_and_dtype():
    from iseg_amd.metrics.mean_iou import get_per_class_miou, per_class_miou_to_mean_miou

    g = torch.Generator().manual_seed(3)
    cm = torch.randint(0, 50, (4, 6, 6), generator=g)
    cm[:, 2, :] = 0
    cm[:, :, 2] = 0      # a class that never occurs: its denominator is 0
    iou, nv = get_per_class_miou(cm)
    old_iou, old_nv = _old_get_per_class_miou(cm)
    assert iou.dtype == torch.float64 and torch.equal(iou, old_iou) and torch.equal(nv, old_nv) and (nv == 5).all() and (iou[:, 2] == 0).all()
    for b in range(4):
        i1, n1 = get_per_class_miou(cm[b])
        assert torch.equal(i1, iou[b]) and torch.equal(n1, nv[b])
    two = cm.reshape(2, 2, 6, 6)
    assert torch.equal(get_per_class_miou(two)[0], iou.reshape(2, 2, 6))
    # rows and columns swapped = the transposed matrix (IoU is symmetric in the two sums, so the values agree with the plain call too)
    si, sn = get_per_class_miou(cm, row_axis=-1, col_axis=-2)
    ti, tn = get_per_class_miou(cm.transpose(-1, -2))
    assert torch.equal(si, ti) and torch.equal(sn, tn)
    fi, fn = get_per_class_miou(cm, dtype=torch.float32)
    assert fi.dtype == torch.float32 and fn.dtype == torch.float32 and torch.allclose(fi.double(), iou, rtol=1e-6, atol=0) and torch.equal(fn.double(), nv)
    di, dn = get_per_class_miou(cm.float(), dtype=torch.float64)
    assert di.dtype == torch.float64 and torch.equal(di, iou)      # counts below 2^24: the float32 sums are exact
    assert per_class_miou_to_mean_miou(iou, nv).shape == (4,)


# ---- the exponent and the fixed-point error bound --------------------------------------------------------------------------------------
def test_weight_exponent():
    from iseg_amd.kernels import confusion_weight_exponent as e

    big = float(np.finfo(np.float32).max)
    tiny = float(np.float32(2.0 ** -149))
    for f in (e, R.weight_exponent):
        assert f(0.0) == 0 and f(1.0) == 37 and f(0.75) == 38 and f(2.0) == 36
        assert f(big) == 38 - 128 and f(tiny) == 38 + 148
        for m in (1.0, 0.75, 3.0e-5, 12345.678, big, tiny, float(np.float32(1e-40))):
            assert 2.0 ** 37 <= m * 2.0 ** f(m) < 2.0 ** 38
    with pytest.raises(ValueError):
        e(float("nan"))
    with pytest.raises(ValueError):
        e(float("inf"))


def test_fixed_point_emulation_stays_inside_the_bound():
    """2^18 elements, C = 5, Gaussian weights times 10^U(-6, 3): |got - ref64| <= 2^-23 |ref64| + k max|w| 2^-38 in every bin"""
    lab, prd, w = R.dynamic_range_case()
    got, counters, w_exp = R.fixed_point_matrix(lab, prd, 5, w)
    ref, bound = R.fixed_point_bound(lab, prd, 5, w)
    assert counters[:5].tolist() == [0] * 5 and counters[5] > 0      # nothing rejected; most weights are rounded
    assert 2.0 ** 37 <= float(np.abs(w).max()) * 2.0 ** w_exp < 2.0 ** 38
    ratio = np.abs(got - ref) / bound
    print("worst ratio to the bound", ratio.max())
    assert (ratio <= 1.0).all()
    # and no bin comes near 2^62
    assert np.abs(R.kernel_counts(lab, prd, 5, w, w_exp)[0]).max() < 2 ** 62


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
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
    header = _header()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(dll, name), name
        res, args = hip.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    assert "confusion.hip" in build.SOURCES
    for macro, value in (("ISEG_CM_W_NONE", kernels.CM_W_NONE), ("ISEG_CM_W_U8", kernels.CM_W_U8), ("ISEG_CM_W_F32", kernels.CM_W_F32),
                         ("ISEG_CM_SLICE", kernels.CM_SLICE), ("ISEG_CM_GRID_CAP", kernels.CM_GRID_CAP), ("ISEG_CM_F32_MAX_N", kernels.CM_F32_MAX_N)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", header).group(1)) == value, macro
    assert (R.SLICE, R.GRID_CAP, R.F32_MAX_N) == (kernels.CM_SLICE, kernels.CM_GRID_CAP, kernels.CM_F32_MAX_N)


def test_no_workspace_function(hip):
    """cm and counters are all the launcher needs: nothing for the workspace ledger of tests/test_guarded_memory_host.py"""
    names = set(re.findall(r"\b(iseg_[a-z0-9_]+)\s*\(", _header())) | set(hip.SIGNATURES)
    assert sorted(n for n in names if "confusion" in n and n != "iseg_argmax_confusion" and n != "iseg_softmax_ce_confusion") == sorted(ENTRY_POINTS)
    assert not [n for n in names if "confusion" in n and n.endswith("_workspace_bytes")]


@pytest.mark.parametrize("Cc,want", [(0, 0), (1, 1), (256, 1), (257, 0)])
def test_supported_class_counts(hip, Cc, want):
    from iseg_amd import kernels

    for wmode in (0, 1, 2):
        assert hip.lib().iseg_confusion_supported(Cc, wmode) == want
        assert kernels.confusion_supported(Cc, wmode) == bool(want)


@pytest.mark.parametrize("wmode,want", [(-1, 0), (0, 1), (2, 1), (3, 0)])
def test_supported_weight_modes(hip, wmode, want):
    assert hip.lib().iseg_confusion_supported(21, wmode) == want


class Buf:
    """a zeroed, 256-byte aligned host buffer"""

    def __init__(self, nbytes=4096):
        self.raw = C.create_string_buffer(nbytes + 256)
        self.ptr = (C.addressof(self.raw) + 255) // 256 * 256


def _refusals():
    """name -> (labels, preds, weights, wmode, w_exp, batch, n, C, cm, counters) with True standing for a small host buffer"""
    ok = dict(labels=True, preds=True, weights=None, wmode=0, w_exp=0, batch=1, n=8, C=3, cm=True, counters=True)
    cases = {
        "null_labels": dict(labels=None), "null_preds": dict(preds=None), "null_cm": dict(cm=None), "null_counters": dict(counters=None),
        "batch_zero": dict(batch=0), "batch_negative": dict(batch=-2), "n_zero": dict(n=0), "n_negative": dict(n=-1),
        "C_zero": dict(C=0), "C_257": dict(C=257), "wmode_3": dict(wmode=3, weights=True), "wmode_negative": dict(wmode=-1, weights=True),
        "u8_without_weights": dict(wmode=1), "f32_without_weights": dict(wmode=2),
    }
    return {k: {**ok, **v} for k, v in cases.items()}


@pytest.mark.skipif(torch.cuda.is_available(), reason="passes host buffers to the launcher: only where no kernel could ever receive them")
@pytest.mark.parametrize("case", sorted(_refusals()))
def test_bad_arguments_are_refused_before_any_launch(hip, case):
    a = _refusals()[case]
    bufs = {k: (Buf().ptr if a[k] else None) for k in ("labels", "preds", "weights", "cm", "counters")}
    status = hip.lib().iseg_confusion_batched(bufs["labels"], bufs["preds"], bufs["weights"], a["wmode"], a["w_exp"], a["batch"], a["n"], a["C"], 0, 255,
                                              bufs["cm"], 0, bufs["counters"], None)
    message = hip.last_error()
    assert status == -1, (case, status, message)
    assert message.startswith("iseg_confusion_batched:"), message


@pytest.mark.skipif(torch.cuda.is_available(), reason="passes host buffers to the launcher: only where no kernel could ever receive them")
def test_f32_weights_past_2_24_elements_are_unsupported_before_any_memory_is_touched(hip):
    b = [Buf() for _ in range(5)]
    status = hip.lib().iseg_confusion_batched(b[0].ptr, b[1].ptr, b[2].ptr, 2, 0, 1, (1 << 24) + 1, 3, 0, 255, b[3].ptr, 0, b[4].ptr, None)
    assert status == -3 and hip.last_error().startswith("iseg_confusion_batched:") and "2^24" in hip.last_error()
    assert hip.lib().iseg_confusion_absmax_f32(None, 8, b[0].ptr, None) == -1 and hip.last_error().startswith("iseg_confusion_absmax_f32:")


def test_wrappers_refuse_host_tensors(hip):
    from iseg_amd import kernels
    from iseg_amd.metrics.mean_iou import get_batch_class_confusion_matrix, get_class_confusion_matrix

    y = torch.zeros(2, 6, dtype=torch.int32)
    with pytest.raises(hip.HipCallError):
        kernels.confusion_batched(y, y, 3)
    with pytest.raises(hip.HipCallError):
        kernels.confusion_absmax(torch.ones(4))
    with pytest.raises(hip.HipCallError):
        get_class_confusion_matrix(y, y, 3)
    with pytest.raises(hip.HipCallError):
        get_batch_class_confusion_matrix(y, y, 3)
    with pytest.raises(ValueError):
        kernels.confusion_batched(y, y.reshape(3, 4), 3)


def test_launcher_arithmetic_of_the_restatement():
    """the shapes the GPU tests lean on"""
    assert R.grid(1, 1) == (1, 1, 1, 1) and R.grid(3, 3 * R.SLICE + 17) == (4, 3, 4, 1) and R.grid(16, 512 * 512) == (64, 16, 64, 1)
    gx, gy, slices, trips = R.grid(1, (1 << 24) + 5)
    assert (gx, gy, slices, trips) == (1024, 1, 4097, 5) and trips * R.SLICE * 255 < 2 ** 32
    assert [R.grid_cap(C, R.W_NONE) for C in (1, 21, 101, 102, 116, 117, 143, 144, 202, 203, 256)] == [1024] * 3 + [768] * 2 + [512] * 2 + [256] * 4
    assert [R.grid_cap(C, R.W_F32) for C in (21, 71, 72, 82, 83, 101, 102, 256)] == [1024, 1024, 768, 768, 512, 512, 256, 256] and R.GRID_CAP == 1024
    assert R.grid(1, 600 * R.SLICE, 150, R.W_U8) == (256, 1, 600, 3) and R.grid(300, 5 * R.SLICE, 256, R.W_F32) == (1, 256, 5, 5)
    assert R.route(202, R.W_U8) == (1, 202, "lds") and R.route(203, R.W_NONE)[0] == 2 and R.route(256, R.W_NONE) == (2, 128, "lds")
    assert R.route(143, R.W_F32)[0] == 1 and R.route(144, R.W_F32)[0] == 2 and R.route(202, R.W_F32)[0] == 2 and R.route(203, R.W_F32)[0] == 3
    assert R.route(246, R.W_F32)[0] == 3 and R.route(247, R.W_F32)[0] == 4 and R.route(256, R.W_F32) == (4, 64, "lds")
    assert math.floor((2 ** 32 - 1) / 255) == 16_843_009
