"""SOD metrics on the host: the fp64 restatement (tests/sod_metrics_ref.py) against answers worked by hand and, where SciPy imports, against
SciPy's distance transform and convolution; the product's surface (package, class names, get_config, reset_state, result accessors) and the
composed route (ISEG_SODMETRICS_FUSED=0) against the restatement.  The numbers through the kernels: tests/test_sod_metrics_gpu.py."""
import numpy as np
import pytest
import torch

from tests import sod_metrics_ref as R


def _img(h, w, seed, density=0.3):
    rng = np.random.default_rng(seed)
    return rng.random((h, w)).astype(np.float32), rng.random((h, w)) < density


def test_perfect_prediction():
    _, gt = _img(12, 15, 0)
    m = R.all_metrics(gt.astype(np.float32), gt)
    assert m["mae"] == 0.0 and m["fm_adp"] == 1.0
    # E: every pixel is perfectly aligned (enhanced value 1), and the reference divides the sum by size - 1 (sod_metrics.py:596), so its
    # "1" is size / (size - 1)
    assert abs(m["sm"] - 1.0) < 1e-12 and abs(m["em_adp"] * (gt.size - 1.0) / gt.size - 1.0) < 1e-12
    assert abs(m["wfm"] - 1.0) < 1e-12
    # every threshold 1..255 binarises a {0, 1} map to gt itself
    assert np.allclose(m["em_curve"][:255], m["em_adp"], atol=1e-12) and np.all(m["fm_curve"][1:256] == 1.0)
    assert np.all(m["precision"][1:256] == 1.0) and np.all(m["recall"][1:] == 1.0) and m["fm_curve"][0] == 0.0


def test_inverted_prediction():
    _, gt = _img(12, 15, 1)
    m = R.all_metrics((~gt).astype(np.float32), gt)
    assert m["mae"] == 1.0 and m["fm_adp"] == 0.0 and m["ngefg"] == 0
    # E at an inverted binarisation: every pixel has align = 2ab/(a^2+b^2) with a, b of opposite sign and |a| = |b| -> -1 -> enhanced 0
    assert m["em_adp"] < 1e-12
    assert np.all(m["precision"][1:256] == 0.0) and np.all(m["recall"][1:256] == 0.0) and np.all(m["fm_curve"][:256] == 0.0)
    # weighted F: E = 1 everywhere; only the zero padding of the Gaussian lets EA < 1 next to the border, so an interior foreground scores 0
    gi = np.zeros((12, 15), bool)
    gi[4:8, 5:10] = True
    assert R.weighted_f((~gi).astype(np.float32), gi) < 1e-12


def test_all_background_and_all_foreground_gt():
    p, _ = _img(9, 11, 2)
    bg, fg = np.zeros((9, 11), bool), np.ones((9, 11), bool)
    mb, mf = R.all_metrics(p, bg), R.all_metrics(p, fg)
    mean = p.astype(np.float64).mean()
    assert abs(mb["sm"] - (1.0 - mean)) < 1e-15 and abs(mf["sm"] - mean) < 1e-15
    assert mb["wfm"] == 0.0 and mb["fm_adp"] == 0.0 and mb["centroid"] == (int(np.round(4.5)) + 1, int(np.round(5.5)) + 1) == (5, 7)
    # all background: E = (#prediction-background) / (size - 1); all foreground: (#prediction-foreground) / (size - 1)
    nge = int((p >= R.adaptive_threshold(p)).sum())
    assert abs(mb["em_adp"] - (99 - nge) / 98.0) < 1e-12 and abs(mf["em_adp"] - nge / 98.0) < 1e-12
    assert np.all(mb["recall"] == 0.0) and np.all(mb["precision"] == 0.0)
    assert mf["recall"][256] == 1.0 and mf["precision"][256] == 1.0


def test_constant_prediction():
    _, gt = _img(10, 10, 3)
    p = np.full((10, 10), 0.25, np.float32)
    m = R.all_metrics(p, gt)
    n = int(gt.sum())
    assert m["thr"] == np.float32(0.5) and m["nge"] == 0 and m["fm_adp"] == 0.0
    assert abs(m["mae"] - (0.75 * n + 0.25 * (100 - n)) / 100.0) < 1e-15
    assert m["hist_fg"][63] == n and m["hist_bg"][63] == 100 - n      # int(0.25 * 255) = 63
    # object term: std 0 -> 2m / (m^2 + 1); region term: sigma_x = sigma_xy = 0 -> alpha = 0, beta != 0 -> 0 in every mixed quadrant
    y = n / 100.0
    obj = y * 2 * 0.25 / (0.0625 + 1 + R.EPS) + (1 - y) * 2 * 0.75 / (0.5625 + 1 + R.EPS)
    assert abs(m["sm"] - 0.5 * obj) < 1e-12


def test_written_out_4x4():
    """gt: the middle 2 x 2 block; pred: 1 on three of its pixels, 0.5 on the fourth, 0.2 on one background pixel, else 0"""
    gt = np.zeros((4, 4), bool)
    gt[1:3, 1:3] = True
    p = np.zeros((4, 4), np.float32)
    p[1, 1] = p[1, 2] = p[2, 1] = 1.0
    p[2, 2] = 0.5
    p[0, 0] = 0.2
    m = R.all_metrics(p, gt)
    fg = np.zeros(256, np.int64)
    fg[255], fg[127] = 3, 1           # int(0.5 * 255) = 127
    bg = np.zeros(256, np.int64)
    bg[0], bg[51] = 11, 1             # int(0.2f * 255) = 51
    assert np.array_equal(m["hist_fg"], fg) and np.array_equal(m["hist_bg"], bg)
    assert m["centroid"] == (3, 3)    # rows {1,1,2,2} -> 1.5 -> 2 (half to even), + 1
    assert m["nfg"] == 4 and abs(m["mae"] - 0.7 / 16) < 1e-8
    assert m["thr"] == np.float32(2 * (3.7 / 16)) or abs(float(m["thr"]) - 0.4625) < 1e-7
    assert (m["nge"], m["ngefg"]) == (4, 4) and m["fm_adp"] == 1.0
    # curves: index i of the 257-point curves is threshold 256 - i
    tp = np.zeros(257)
    tp[1:] = 3
    tp[129:] = 4                      # threshold 127 is index 129
    ps = tp.copy()
    ps[205:] += 1                     # threshold 51 is index 205
    ps[256] += 11
    prec = np.where(ps == 0, 0, tp / np.maximum(ps, 1))
    assert np.allclose(m["precision"], prec, atol=1e-15) and np.allclose(m["recall"], tp / 4.0, atol=1e-15)
    f = 1.3 * prec * (tp / 4) / np.where(prec * tp == 0, 1, 0.3 * prec + tp / 4)
    assert np.allclose(m["fm_curve"], f, atol=1e-15)
    assert abs(m["em_curve"][128] - 16 / 15.0) < 1e-12 and abs(m["em_adp"] - 16 / 15.0) < 1e-12      # a perfect binarisation: size / (size - 1)


def test_one_foreground_pixel_distance_transform():
    gt = np.zeros((7, 9), bool)
    gt[2, 5] = True
    d2, nn = R.edt(gt)
    yy, xx = np.mgrid[:7, :9]
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), np.hypot(yy - 2, xx - 5)) and np.all(nn == 2 * 9 + 5)


def test_distance_tie_takes_the_smallest_row_major_index():
    gt = np.zeros((3, 5), bool)
    gt[0, 4] = gt[2, 0] = gt[1, 1] = gt[1, 3] = True
    d2, nn = R.edt(gt)
    assert d2[1, 2] == 1 and nn[1, 2] == 1 * 5 + 1      # (1,1) and (1,3) tie
    assert d2[0, 2] == 2 and nn[0, 2] == 1 * 5 + 1      # (1,1), (1,3) at 2; (0,4) at 4


def test_degenerate_quadrants():
    """the centroid on the last row and column: three quadrants have no pixels and contribute 0; a one-pixel quadrant has variances 0"""
    gt = np.zeros((5, 6), bool)
    gt[4, 5] = True
    p, _ = _img(5, 6, 4)
    assert R.centroid(gt) == (5, 6)
    s = R.s_measure(p, gt)
    assert np.isfinite(s)
    pd, g = p.astype(np.float64), gt.astype(np.float64)
    obj = R._s_object(pd[gt]) / 30.0 + R._s_object(1.0 - pd[~gt]) * 29.0 / 30.0
    assert abs(s - max(0.0, 0.5 * obj + 0.5 * R.ssim(pd, g) * 1.0)) < 1e-15
    assert R.ssim(np.zeros((0, 3)), np.zeros((0, 3))) == 0.0
    assert R.ssim(np.array([[0.3]]), np.array([[1.0]])) == 1.0 and R.ssim(np.array([[0.0]]), np.array([[0.0]])) == 1.0
    gt2 = np.zeros((5, 6), bool)
    gt2[3, 4] = gt2[4, 4] = True      # cy = round(3.5) + 1 = 5 (half to even: 4), cx = 5: the right column is one pixel wide
    assert R.centroid(gt2) == (5, 5) and np.isfinite(R.s_measure(p, gt2))


def test_prepare_data_is_mapminmax_in_fp32():
    rng = np.random.default_rng(5)
    u = rng.integers(7, 201, (6, 8)).astype(np.uint8)
    g = rng.integers(0, 256, (6, 8)).astype(np.uint8)
    p, gt = R.prepare_data(u, g)
    assert p.dtype == np.float32 and p.min() == 0.0 and p.max() == 1.0 and np.array_equal(gt, g > 128)
    c, _ = R.prepare_data(np.full((3, 3), 51, np.uint8), g[:3, :3])
    assert np.all(c == np.float32(51) / np.float32(255))


def test_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(6)
    for shape, density in (((37, 53), 0.02), ((37, 53), 0.4), ((64, 48), 0.001), ((5, 90), 0.1)):
        gt = rng.random(shape) < density
        gt[rng.integers(shape[0]), rng.integers(shape[1])] = True
        d2, _ = R.edt(gt)
        dist = ndi.distance_transform_edt(~gt)
        assert np.array_equal(d2, np.rint(dist * dist).astype(np.int64))
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), dist)
        # the whole weighted F-measure, the prediction constant over the foreground so that the tie choice cannot matter
        p = rng.random(shape).astype(np.float32)
        p[gt] = np.float32(0.8)
        dist, ind = ndi.distance_transform_edt(~gt, return_indices=True)
        sci = (np.rint(dist * dist).astype(np.int64), ind[0].astype(np.int64) * shape[1] + ind[1])
        assert abs(R.weighted_f(p, gt) - R.weighted_f(p, gt, dist=sci)) < 1e-15
    a = rng.random((20, 31))
    assert np.allclose(R.convolve7(a, R.gaussian7()), ndi.convolve(a, R.gaussian7(), mode="constant", cval=0.0), atol=1e-15, rtol=0)


# ---- the product's surface ---------------------------------------------------------------------------------------------------------------
def test_package_exports_the_reference_names():
    import iseg_amd.metrics.sod as sod

    for n in ("TFSmeasureMetric", "TFEmeasureMetric", "TFFmeasureMetric", "TFWeightedFmeasureMetric", "TFMAEMetric"):
        assert hasattr(sod, n)
    from iseg_amd.metrics.sod import sod_metric_utils, sod_metrics  # noqa: F401

    assert sod_metric_utils.EPS == R.EPS


def test_get_config_and_defaults():
    from iseg_amd.metrics.sod import TFEmeasureMetric, TFFmeasureMetric, TFMAEMetric, TFSmeasureMetric, TFWeightedFmeasureMetric

    assert TFMAEMetric().get_config()["name"] == "mae" and TFEmeasureMetric().get_config()["name"] == "em"
    assert TFSmeasureMetric().get_config() == {"name": "sm", "dtype": "float32", "alpha": 0.5}
    assert TFFmeasureMetric().get_config() == {"name": "fm", "dtype": "float32", "beta": 0.3}
    assert TFWeightedFmeasureMetric().get_config() == {"name": "wfm", "dtype": "float32", "beta": 1.0}
    assert TFSmeasureMetric(alpha=0.7, name="s").get_config() == {"name": "s", "dtype": "float32", "alpha": 0.7}


def test_fused_route_has_no_host_path():
    from iseg_amd import _hip
    from iseg_amd.metrics.sod import TFMAEMetric

    with pytest.raises((_hip.HipCallError, _hip.HipLibraryMissing)):
        TFMAEMetric().update_state(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.bool))


def _classes():
    from iseg_amd.metrics.sod import TFEmeasureMetric, TFFmeasureMetric, TFMAEMetric, TFSmeasureMetric, TFWeightedFmeasureMetric

    return TFMAEMetric(), TFSmeasureMetric(), TFEmeasureMetric(), TFFmeasureMetric(), TFWeightedFmeasureMetric()


def test_composed_route_results_accessors_and_reset(monkeypatch):
    """the classes on host tensors through the composed route: result() / adaptive_result() / curves against the restatement, [B,H,W] input
    against image-by-image updates, safe_divide on an empty state, reset_state"""
    from iseg_amd import nn
    from iseg_amd.metrics.sod import SodMetricSet

    monkeypatch.setenv("ISEG_SODMETRICS_FUSED", "0")
    monkeypatch.setitem(nn._POLICY, "device", torch.device("cpu"))
    imgs = [_img(13, 17, 10 + k) for k in range(3)]
    imgs[1] = (imgs[1][0], np.zeros((13, 17), bool))
    last = np.zeros((13, 17), bool)
    last[12, 16] = True      # the centroid on the last row and column: three quadrants without pixels (the N <= 1 rule, through the product)
    imgs[2] = (imgs[2][0], last)
    want = [R.all_metrics(p, g) for p, g in imgs]
    mae, sm, em, fm, wfm = ms = _classes()
    for m in ms:
        assert float(m.result()) == 0.0      # safe_divide: 0 / 0 -> 0
    P = torch.from_numpy(np.stack([p for p, _ in imgs]))
    G = torch.from_numpy(np.stack([g for _, g in imgs]))
    for m in ms:
        m.update_state(P[0], G[0])
        m.update_state(P[1:], G[1:])
    mean = lambda k: np.mean([w[k] for w in want], axis=0)      # noqa: E731
    assert abs(float(mae.result()) - mean("mae")) < 1e-6 and abs(float(sm.result()) - mean("sm")) < 1e-6
    assert abs(float(wfm.result()) - mean("wfm")) < 1e-6
    assert abs(float(em.result()) - mean("em_curve").mean()) < 1e-6 and abs(float(fm.result()) - mean("fm_curve").mean()) < 1e-6
    assert abs(float(em.adaptive_result()) - mean("em_adp")) < 1e-6 and abs(float(fm.adaptive_result()) - mean("fm_adp")) < 1e-6
    assert em.curve_result().shape == (256,) and fm.curve_result().shape == (257,)
    assert np.allclose(em.curve_result().numpy(), mean("em_curve"), atol=1e-6) and np.allclose(fm.curve_result().numpy(), mean("fm_curve"), atol=1e-6)
    assert np.allclose(fm.precision_curve().numpy(), mean("precision"), atol=1e-6) and np.allclose(fm.recall_curve().numpy(), mean("recall"), atol=1e-6)
    assert mae.result().dtype == torch.float32
    # the state itself, fp64: 1e-12
    assert abs(float(sm._set.state[1]) / 3 - mean("sm")) < 1e-12 and abs(float(wfm._set.state[4]) / 3 - mean("wfm")) < 1e-12
    assert np.isfinite(float(sm._set.state[1]))
    # a one-pixel quadrant: gt on the last two rows of the second-last column of a 5 x 6 image (centroid (5, 5): the right column is 5 x 1, the
    # bottom row 1 x 5 ... and the corner ONE pixel)
    g2 = np.zeros((5, 6), bool)
    g2[3, 4] = g2[4, 4] = True
    p2, _ = _img(5, 6, 4)
    one = _classes()[1]
    one.update_state(torch.from_numpy(p2), torch.from_numpy(g2))
    assert abs(float(one._set.state[1]) - R.s_measure(p2, g2)) < 1e-12
    # a set shares one state, and its members are updated through it only
    st = SodMetricSet(*_classes())
    st.update_state(P, G)
    assert float(st.metrics[1].result()) == float(sm.result()) and int(st.count) == 3
    with pytest.raises(RuntimeError):
        st.metrics[0].update_state(P, G)
    assert int(st.count) == 3
    for m in ms:
        m.reset_state()
        assert float(m.result()) == 0.0 and int(m._set.count) == 0
    # uint8 inputs with normalize=True
    rng = np.random.default_rng(20)
    u, g8 = rng.integers(3, 250, (13, 17)).astype(np.uint8), rng.integers(0, 256, (13, 17)).astype(np.uint8)
    pn, gn = R.prepare_data(u, g8)
    sm.update_state(torch.from_numpy(u), torch.from_numpy(g8), normalize=True)
    assert abs(float(sm._set.state[1]) - R.s_measure(pn, gn)) < 1e-12
    with pytest.raises(ValueError):
        sm.update_state(P[0], G[0, :5])
