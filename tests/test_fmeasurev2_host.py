"""FmeasureV2 on the host: the restatement (tests/fmeasurev2_ref.py) against answers worked by hand on a 2 x 3 image, the product's surface (names,
aliases, defaults, get_config, refusals) and the composed route (ISEG_SODFMV2_FUSED=0) on CPU tensors against the restatement.  The numbers through
the kernel: tests/test_fmeasurev2_gpu.py."""
import numpy as np
import pytest
import torch

from tests import fmeasurev2_ref as R

PRED = np.array([[1.0, 0.4, 0.6], [0.0, 0.2, 0.0]], np.float32)
GT = np.array([[1, 1, 0], [0, 0, 0]], bool)
# bins int(p * 255.0f): 255, 102, 153 / 0, 51, 0.  mean = 2.2 / 6, threshold = 0.7333: only the 1.0 passes.  p > 0.5: the 1.0 (fg) and the 0.6 (bg).
ADAPTIVE = dict(iou=1 / 2, specificity=1.0, dice=2 / 3, overall_accuracy=5 / 6, kappa=1 / 3, precision=1.0, recall=0.5, fpr=0.0, ber=0.25,
                fmeasure=1.3 * 0.5 / (0.3 + 0.5))                  # tp, fp, tn, fn = 1, 0, 4, 1; kappa: p_e = (1*2 + 5*5) / 36
BINARY = dict(iou=1 / 3, specificity=3 / 4, dice=0.5, overall_accuracy=4 / 6, kappa=0.25, precision=0.5, recall=0.5, fpr=0.25, ber=0.375,
              fmeasure=0.5)                                        # 1, 1, 3, 1; kappa: p_e = (2*2 + 4*4) / 36, (2/3 - 5/9) / (4/9)
AT_153 = dict(iou=2 / 3, specificity=3 / 4, dice=4 / 5, overall_accuracy=5 / 6, kappa=(5 / 6 - 21 / 36) / (15 / 36), precision=2 / 3, recall=1.0,
              fpr=0.25, ber=0.125, fmeasure=1.3 * (2 / 3) / (0.2 + 1.0))      # threshold 102: 2, 1, 3, 0; p_e = (3*2 + 3*5) / 36
AT_255 = dict(iou=2 / 6, specificity=0.0, dice=4 / 8, overall_accuracy=2 / 6, kappa=0.0, precision=2 / 6, recall=1.0, fpr=1.0, ber=0.5,
              fmeasure=1.3 * (1 / 3) / (0.1 + 1.0))                # threshold 0: 2, 4, 0, 0; p_e = (6*2 + 0*2) / 36 = oa


def test_counts_of_the_written_out_image():
    w = R.integers(PRED, GT)
    fg, bg = np.zeros(256, np.int64), np.zeros(256, np.int64)
    fg[255] = fg[102] = 1
    bg[153] = bg[51] = 1
    bg[0] = 2
    assert np.array_equal(w["hist_fg"], fg) and np.array_equal(w["hist_bg"], bg)
    assert (w["nfg"], w["nge"], w["ngefg"], w["n05"], w["n05fg"]) == (2, 1, 1, 2, 1)
    assert abs(float(w["thr"]) - 2.2 / 3) < 1e-7
    dyn, adp, bny = R.counts(PRED, GT)
    assert adp == (1, 0, 4, 1) and bny == (1, 1, 3, 1)
    # index i is threshold 255 - i: TP steps at threshold 102 (i = 153); FP at 153 (i = 102), 51 (i = 204) and 0 (i = 255)
    tp = np.where(np.arange(256) >= 153, 2, 1)
    fp = np.select([np.arange(256) >= 255, np.arange(256) >= 204, np.arange(256) >= 102], [4, 2, 1], 0)
    assert np.array_equal(dyn[0], tp) and np.array_equal(dyn[1], fp) and np.array_equal(dyn[2], 4 - fp) and np.array_equal(dyn[3], 2 - tp)


def test_every_handler_and_mode_of_the_written_out_image():
    m = R.all_handlers(PRED, GT)
    assert m["binary_counts"] == (1, 1, 3, 1)
    for kind in R.KINDS:
        assert abs(m[kind]["adaptive"] - ADAPTIVE[kind]) < 1e-15, kind
        assert abs(m[kind]["binary"] - BINARY[kind]) < 1e-15, kind
        curve = m[kind]["dynamic"]
        assert curve.shape == (256,) and curve.dtype == np.float64
        assert abs(curve[0] - ADAPTIVE[kind]) < 1e-15 and abs(curve[101] - ADAPTIVE[kind]) < 1e-15, kind      # thresholds 255..154: 1, 0, 4, 1
        assert abs(curve[102] - BINARY[kind]) < 1e-15 and abs(curve[152] - BINARY[kind]) < 1e-15, kind        # thresholds 153..103: 1, 1, 3, 1
        assert abs(curve[153] - AT_153[kind]) < 1e-15 and abs(curve[203] - AT_153[kind]) < 1e-15, kind
        assert abs(curve[255] - AT_255[kind]) < 1e-15, kind
    assert abs(R.compute_metric("fmeasure", 1, 1, 3, 1, beta=1.0) - 0.5) < 1e-15 and abs(R.compute_metric("fmeasure", 2, 1, 3, 0, beta=1.0) - 0.8) < 1e-15


def test_all_background_and_all_foreground_gt():
    bg, fg = np.zeros((2, 3), bool), np.ones((2, 3), bool)
    mb, mf = R.all_handlers(PRED, bg), R.all_handlers(PRED, fg)
    assert mb["binary_counts"] == (0, 2, 4, 0) and mf["binary_counts"] == (2, 0, 0, 4)
    # no foreground: every quotient with tp on top is 0, recall is 0 / 0 -> 0; kappa: p_e = (2*0 + 4*4) / 36
    want_b = dict(iou=0.0, specificity=4 / 6, dice=0.0, overall_accuracy=4 / 6, kappa=(2 / 3 - 4 / 9) / (5 / 9), precision=0.0, recall=0.0, fpr=2 / 6,
                  ber=1.0 - 0.5 * (4 / 6), fmeasure=0.0)
    # no background: specificity and fpr are 0 / 0 -> 0; kappa: p_e = (2*6 + 4*2) / 36, (1/3 - 5/9) / (4/9)
    want_f = dict(iou=2 / 6, specificity=0.0, dice=0.5, overall_accuracy=2 / 6, kappa=-0.5, precision=1.0, recall=1 / 3, fpr=0.0, ber=1.0 - 0.5 / 3,
                  fmeasure=13 / 19)
    for kind in R.KINDS:
        assert abs(mb[kind]["binary"] - want_b[kind]) < 1e-15 and abs(mf[kind]["binary"] - want_f[kind]) < 1e-15, kind
        assert np.all(np.isfinite(mb[kind]["dynamic"])) and np.all(np.isfinite(mf[kind]["dynamic"])), kind
    # threshold 0 on the all-foreground gt: tp = 6 and nothing else -> p_e = 36 / 36 and Kappa's last division is 0 / 0 -> 0
    assert mf["kappa"]["dynamic"][255] == 0.0 and mf["overall_accuracy"]["dynamic"][255] == 1.0
    # all background, thresholds 254..154 pass the 1.0 alone: 0, 1, 5, 0 -> p_e = (1*0 + 5*5) / 36, kappa = (30 - 25) / (36 - 25)
    assert abs(mb["kappa"]["dynamic"][50] - 5 / 11) < 1e-15 and mb["iou"]["dynamic"][50] == 0.0 and mb["precision"]["dynamic"][50] == 0.0
    # nothing predicted and nothing to find: tn = 6 alone -> the same 0 / 0
    assert R.compute_metric("kappa", 0, 0, 6, 0) == 0.0 and R.compute_metric("overall_accuracy", 0, 0, 6, 0) == 1.0
    assert R.compute_metric("iou", 0, 0, 0, 0) == 0.0 and R.compute_metric("kappa", 0, 0, 0, 0) == 0.0


# ---- the product's surface ---------------------------------------------------------------------------------------------------------------
NAMES = dict(TFIOUHandler="iou", TFSpecificityHandler="specificity", TFDICEHandler="dice", TFOverallAccuracyHandler="overall_accuracy",
             TFKappaHandler="kappa", TFPrecisionHandler="precision", TFRecallHandler="recall", TFFPRHandler="fpr", TFBERHandler="ber",
             TFFmeasureHandler="fmeasure")


def test_package_exports_the_reference_names_aliases_and_defaults():
    import iseg_amd.metrics.sod as sod
    from iseg_amd.metrics.sod import fmeasurev2  # noqa: F401

    for cls, name in NAMES.items():
        h = getattr(sod, cls)(True, False)
        assert issubclass(getattr(sod, cls), sod.TFBaseHandler) and h.name == name and getattr(sod, cls).__name__ == cls
        assert (h.with_dynamic, h.with_adaptive, h.with_binary, h.sample_based) == (True, False, False, True)
        assert R.KINDS[h.KIND] == name
    assert sod.TFTNRHandler is sod.TFSpecificityHandler and sod.TFTPRHandler is sod.TFRecallHandler and sod.TFSensitivityHandler is sod.TFRecallHandler
    assert sod.TFFmeasureHandler(True, True).beta == 0.3 and sod.TFFmeasureV2().name == "fmeasure_v2"
    with pytest.raises(TypeError):
        sod.TFIOUHandler(True, True, True)      # with_binary is keyword-only, as in the reference


def test_get_config():
    from iseg_amd.metrics.sod import TFFmeasureHandler, TFFmeasureV2, TFKappaHandler

    assert TFKappaHandler(with_dynamic=True, with_adaptive=False, with_binary=True, sample_based=False).get_config() == {
        "name": "kappa", "dtype": "float32", "with_dynamic": True, "with_adaptive": False, "with_binary": True, "sample_based": False}
    assert TFFmeasureHandler(False, True, beta=1.0, name="f1").get_config() == {
        "name": "f1", "dtype": "float32", "with_dynamic": False, "with_adaptive": True, "with_binary": False, "sample_based": True, "beta": 1.0}
    assert TFFmeasureV2().get_config() == {"name": "fmeasure_v2", "dtype": "float32"}


def test_evaluator_without_handlers_and_member_updates_are_refused(monkeypatch):
    from iseg_amd import nn
    from iseg_amd.metrics.sod import TFBaseHandler, TFFmeasureV2, TFIOUHandler, TFRecallHandler

    monkeypatch.setitem(nn._POLICY, "device", torch.device("cpu"))
    P, G = torch.from_numpy(PRED), torch.from_numpy(GT)
    with pytest.raises(ValueError, match="add your metric handler"):
        TFFmeasureV2().update_state(P, G, normalize=False)
    iou, rec = TFIOUHandler(True, True), TFRecallHandler(True, True)
    ev = TFFmeasureV2({"iou": iou})
    ev.add_handler("rec", rec)
    assert tuple(ev.state.shape) == (2, 264) and ev.state.dtype == torch.float64 and ev.count.dtype == torch.int64
    with pytest.raises(RuntimeError, match="share one state"):
        iou.update_state(P, G, normalize=False)
    with pytest.raises(RuntimeError, match="share one state"):
        rec.reset_state()
    with pytest.raises(ValueError):
        ev.update_state(P, G[:, :2], normalize=False)
    with pytest.raises(NotImplementedError):
        TFBaseHandler(True, True).update_state(P, G, normalize=False)
    with pytest.raises(ValueError):
        TFFmeasureV2({str(k): TFIOUHandler(True, False) for k in range(33)})


def test_fused_route_has_no_host_path():
    from iseg_amd import _hip
    from iseg_amd.metrics.sod import TFIOUHandler

    with pytest.raises((_hip.HipCallError, _hip.HipLibraryMissing)):
        TFIOUHandler(True, True).update_state(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.bool), normalize=False)


def _all_handlers(sample_based=True):
    import iseg_amd.metrics.sod as sod

    return {name: getattr(sod, cls)(True, True, with_binary=True, sample_based=sample_based) for cls, name in NAMES.items()}


def _close32(got, want):
    """result() is fp32: the sum is rounded to fp32 and divided in fp32, two roundings of 2^-24 relative each.  1e-6 of the value's size, and 1e-6
    absolute below 1.  (The reference's Kappa formula is unbounded: -x / (1 - x) on an all-foreground gt with a fraction x predicted.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= 1e-6 * np.maximum(1.0, np.abs(want))))


def _img(h, w, seed, density=0.3):
    rng = np.random.default_rng(seed)
    return rng.random((h, w)).astype(np.float32), rng.random((h, w)) < density


def test_composed_route_against_the_restatement(monkeypatch):
    """the classes on host tensors through the composed route: result() dicts, [B,H,W] input against image-by-image updates, the degenerate gts,
    the dataset-based binary mode, compute_metric, reset_state, uint8 inputs under normalize"""
    from iseg_amd import nn
    from iseg_amd.metrics.sod import TFFmeasureV2, TFKappaHandler
    from iseg_amd.metrics.sod.fmeasurev2 import composed_record

    monkeypatch.setenv("ISEG_SODFMV2_FUSED", "0")
    monkeypatch.setitem(nn._POLICY, "device", torch.device("cpu"))
    imgs = [_img(13, 17, 30 + k) for k in range(4)] + [(PRED, GT)]
    imgs[1] = (imgs[1][0], np.zeros((13, 17), bool))
    imgs[2] = (imgs[2][0], np.ones((13, 17), bool))
    want = [R.all_handlers(p, g) for p, g in imgs]
    # the record of one image, fp64
    table = [(k, 7, 0.3) for k in range(10)]
    for (p, g), w in zip(imgs, want):
        rec = composed_record(torch.from_numpy(p), torch.from_numpy(g), table).numpy()
        for k, kind in enumerate(R.KINDS):
            assert np.max(np.abs(rec[k, :256] - w[kind]["dynamic"])) < 1e-12 and abs(rec[k, 256] - w[kind]["adaptive"]) < 1e-12, kind
            assert abs(rec[k, 257] - w[kind]["binary"]) < 1e-12 and tuple(rec[k, 258:262]) == w["binary_counts"] and not rec[k, 262:].any(), kind
    ev, ds = TFFmeasureV2(_all_handlers()), TFFmeasureV2(_all_handlers(sample_based=False))
    assert ev.result()["iou"]["binary"] == 0.0 and not ev.result()["kappa"]["dynamic"].any()      # safe_divide: 0 / 0 -> 0
    P = torch.from_numpy(np.stack([p for p, _ in imgs[:4]]))
    G = torch.from_numpy(np.stack([g for _, g in imgs[:4]]))
    for e in (ev, ds):
        e.update_state(P[0], G[0], normalize=False)
        e.update_state(P[1:], G[1:], normalize=False)
        e.update_state(torch.from_numpy(PRED), torch.from_numpy(GT), normalize=False)
        assert int(e.count) == 5
    res, dres = ev.result(), ds.result()
    tot = [sum(w["binary_counts"][j] for w in want) for j in range(4)]
    for kind in R.KINDS:
        r = res[kind]
        assert set(r) == {"dynamic", "adaptive", "binary"} and r["dynamic"].shape == (256,) and r["dynamic"].dtype == torch.float32
        assert _close32(r["dynamic"].numpy(), np.mean([w[kind]["dynamic"] for w in want], axis=0)), kind
        assert _close32(float(r["adaptive"]), np.mean([w[kind]["adaptive"] for w in want])), kind
        assert _close32(float(r["binary"]), np.mean([w[kind]["binary"] for w in want])), kind
        assert _close32(float(dres[kind]["binary"]), float(R.compute_metric(kind, *tot))), kind
        assert torch.equal(dres[kind]["dynamic"], r["dynamic"])
    # only the requested modes are reported, and a handler alone owns an evaluator of one
    kap = TFKappaHandler(False, True)
    kap.update_state(torch.from_numpy(PRED), torch.from_numpy(GT), normalize=False)
    assert set(kap.result()) == {"adaptive"} and abs(float(kap.result()["adaptive"]) - 1 / 3) < 1e-6
    assert abs(float(kap.compute_metric(1, 1, 3, 1)) - 0.25) < 1e-15
    kap.reset_state()
    assert float(kap.result()["adaptive"]) == 0.0 and int(kap._evaluator.count) == 0
    ev.reset_state()
    assert int(ev.count) == 0 and not ev.state.any()
    # uint8 inputs: normalize=True is the default
    rng = np.random.default_rng(40)
    u, g8 = rng.integers(3, 250, (13, 17)).astype(np.uint8), rng.integers(0, 256, (13, 17)).astype(np.uint8)
    w = R.all_handlers(*R.S.prepare_data(u, g8))
    ev.update_state(torch.from_numpy(u), torch.from_numpy(g8))
    for kind in R.KINDS:
        assert _close32(ev.result()[kind]["dynamic"].numpy(), w[kind]["dynamic"]), kind
    with pytest.raises(RuntimeError, match="counted images"):
        ev.add_handler("late", TFKappaHandler(True, True))


def test_against_the_reference_classes():
    """one case against the reference's own classes, where TensorFlow and the reference package import"""
    tf = pytest.importorskip("tensorflow", reason="TensorFlow is not installed: the reference's classes cannot run")
    ref = pytest.importorskip("iseg.metrics.sod.fmeasurev2", reason="the reference package (iseg) is not installed")
    p, g = _img(13, 17, 50)
    want = R.all_handlers(p, g)
    for cls, name in NAMES.items():
        h = getattr(ref, cls)(True, True, with_binary=True)
        h.update_state(tf.constant(p), tf.constant(g), normalize=False)
        got = h.result()
        assert np.allclose(got["dynamic"].numpy(), want[name]["dynamic"], atol=1e-6, rtol=0), name
        assert abs(float(got["adaptive"]) - want[name]["adaptive"]) < 1e-6 and abs(float(got["binary"]) - want[name]["binary"]) < 1e-6, name
