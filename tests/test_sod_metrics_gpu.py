"""SOD metrics through the HIP kernels (csrc/sod_metrics.hip), by the C ABI wrapper and by the classes, against the fp64 restatement
tests/sod_metrics_ref.py.

Integers (histograms, foreground count, adaptive counts, centroid, squared distances, nearest indices) must be bit-exact.  Each case asserts
on the CPU, before anything is compared, that no pixel lies within 4 fp32 ulps of the adaptive threshold: a condition on the INPUTS (the
threshold is an fp32 rounding of a mean, and the kernels' fixed-order fp64 mean may differ from NumPy's pairwise one in the last bit); no pixel
is ever left out of a comparison.

Quantities computed only from those integers (E curve, precision / recall / F curves, adaptive E and F): 1e-9 absolute; both sides evaluate
the same few dozen fp64 operations on identical integers and values <= 1, only the operation order (and FMA contraction) differs.

Quantities that rest on float sums (MAE, S-measure, weighted F): FLOAT_BOUND below.  It is 10 x the worst gap measured over the cases of this file
(MAE 1.4e-17, S-measure 3.3e-16, weighted F 1.1e-16): the kernels accumulate in fp64, far below the 1e-6 such a score would be allowed.
"""
import numpy as np
import pytest
import torch

from tests import sod_metrics_ref as R

pytestmark = pytest.mark.gpu

INT_BOUND = 1e-9
FLOAT_BOUND = 4e-15      # measured worst gap 3.3e-16 (S-measure, 16 x 512 x 512): every sum is fp64 and p^2, p - g, 1 - p are exact
WORST = {}


def saliency(B, H, W, seed, density=0.3):
    """near-binary map: ~90 % of the pixels exactly 0 or 1 (right where gt says, mostly), the rest uniform; blobby gt"""
    rng = np.random.default_rng(seed)
    coarse = rng.random((B, H // 8 + 2, W // 8 + 2))
    gt = np.kron(coarse, np.ones((1, 8, 8)))[:, 3:H + 3, 5:W + 5] < density
    p = gt.astype(np.float32)
    wrong = rng.random((B, H, W)) < 0.04
    p[wrong] = 1.0 - p[wrong]
    soft = rng.random((B, H, W)) < 0.1
    p[soft] = rng.random((B, H, W)).astype(np.float32)[soft]
    return p, gt


def uniform(B, H, W, seed, density=0.3):
    rng = np.random.default_rng(seed)
    return (rng.random((B, H, W)) * 0.8).astype(np.float32), rng.random((B, H, W)) < density


def grey(B, H, W, seed):
    rng = np.random.default_rng(seed)
    p, gt = saliency(B, H, W, seed)
    u = np.clip(p * 200.0 + 20.0 + rng.integers(0, 6, (B, H, W)), 0, 255).astype(np.uint8)
    g = np.where(gt, rng.integers(129, 256, (B, H, W)), rng.integers(0, 129, (B, H, W))).astype(np.uint8)
    return u, g


CASES = {
    "odd_37x53_saliency": lambda: saliency(1, 37, 53, 1) + (False,),
    "odd_37x53_uniform": lambda: uniform(1, 37, 53, 2) + (False,),
    "4x128x160_uniform": lambda: uniform(4, 128, 160, 3) + (False,),
    "3x61x67_uint8_normalize": lambda: grey(3, 61, 67, 4) + (True,),
    "2x64x96_uint8_normalize": lambda: grey(2, 64, 96, 5) + (True,),
    "16x512x512_saliency": lambda: saliency(16, 512, 512, 6) + (False,),
    "1x1024x1024_saliency": lambda: saliency(1, 1024, 1024, 7) + (False,),
}


def _as_float(pred, gt, normalize):
    if not normalize:
        return pred, gt
    out = [R.prepare_data(pred[b], gt[b]) for b in range(pred.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _assert_threshold_clear(p):
    for b in range(p.shape[0]):
        thr = R.adaptive_threshold(p[b])
        gap = np.abs(p[b].view(np.int32).astype(np.int64) - int(thr.view(np.int32)))
        assert int(gap.min()) > 4, f"input condition: a pixel of image {b} lies within 4 ulps of the adaptive threshold {thr}"


def _gap(name, got, want, bound):
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))))
    WORST[name] = max(WORST.get(name, 0.0), err)
    print(f"    {name}: max gap {err:.3e}  (bound {bound:.1e})")
    assert np.all(np.isfinite(got)) and err <= bound, (name, err, bound)


@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_restatement(cuda, case):
    from iseg_amd import kernels as K

    pred, gt, normalize = CASES[case]()
    p, g = _as_float(pred, gt, normalize)
    _assert_threshold_clear(p)
    state = torch.zeros(K.SOD_STATE_DOUBLES, dtype=torch.float64, device=cuda)
    count = torch.zeros(1, dtype=torch.int64, device=cuda)
    ints, per, d2, nn = K.sod_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), normalize=normalize, state=state, count=count,
                                      want_ints=True, want_per_image=True, want_dist=True)
    ints, per, d2, nn = ints.cpu().numpy(), per.cpu().numpy(), d2.cpu().numpy(), nn.cpu().numpy()
    B = p.shape[0]
    assert int(count) == B
    print(case)
    total = np.zeros(K.SOD_STATE_DOUBLES)
    for b in range(B):
        w = R.all_metrics(p[b], g[b])
        assert np.array_equal(ints[b, :256], w["hist_fg"]) and np.array_equal(ints[b, 256:512], w["hist_bg"]), "histograms"
        assert ints[b, 512] == w["nfg"] and (ints[b, 513], ints[b, 514]) == (w["nge"], w["ngefg"]), "counts"
        assert (ints[b, 515], ints[b, 516]) == w["centroid"], "centroid"
        assert abs(int(ints[b, 517]) - int(w["thr"].view(np.int32))) <= 1, "adaptive threshold"
        if w["dist"] is not None:
            assert np.array_equal(d2[b], w["dist"][0]), "squared distances"
            assert np.array_equal(nn[b], w["dist"][1]), "nearest foreground index"
        _gap("E adaptive", per[b, 2], w["em_adp"], INT_BOUND)
        _gap("F adaptive", per[b, 3], w["fm_adp"], INT_BOUND)
        _gap("E curve", per[b, 5:261], w["em_curve"], INT_BOUND)
        _gap("F curve", per[b, 261:518], w["fm_curve"], INT_BOUND)
        _gap("precision", per[b, 518:775], w["precision"], INT_BOUND)
        _gap("recall", per[b, 775:1032], w["recall"], INT_BOUND)
        _gap("MAE", per[b, 0], w["mae"], FLOAT_BOUND)
        _gap("S-measure", per[b, 1], w["sm"], FLOAT_BOUND)
        _gap("weighted F", per[b, 4], w["wfm"], FLOAT_BOUND)
        total += per[b]
    # the running state is the images added in order
    assert np.array_equal(state.cpu().numpy(), total)
    print("    worst so far:", {k: f"{v:.2e}" for k, v in WORST.items()})


def _metrics():
    from iseg_amd.metrics.sod import TFEmeasureMetric, TFFmeasureMetric, TFMAEMetric, TFSmeasureMetric, TFWeightedFmeasureMetric

    return [TFMAEMetric(), TFSmeasureMetric(), TFEmeasureMetric(), TFFmeasureMetric(), TFWeightedFmeasureMetric()]


def test_classes_against_the_restatement_and_degenerate_gts(cuda):
    """through the classes: an all-background, an all-foreground and a last-row-and-column gt among ordinary images"""
    from iseg_amd.metrics.sod import SodMetricSet

    p, g = saliency(5, 45, 52, 11)
    g[1] = False
    g[2] = True
    g[3] = False
    g[3, 44, 51] = True
    _assert_threshold_clear(p)
    want = [R.all_metrics(p[b], g[b]) for b in range(5)]
    ms = _metrics()
    st = SodMetricSet(ms)
    st.update_state(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda())
    mean = lambda k: np.mean([w[k] for w in want], axis=0)      # noqa: E731
    state = st.state.cpu().numpy() / 5.0
    _gap("MAE", state[0], mean("mae"), FLOAT_BOUND)
    _gap("S-measure", state[1], mean("sm"), FLOAT_BOUND)
    _gap("weighted F", state[4], mean("wfm"), FLOAT_BOUND)
    mae, sm, em, fm, wfm = ms
    # result() is fp32, as the reference's safe_divide
    assert abs(float(mae.result()) - mean("mae")) < 1e-6 and abs(float(sm.result()) - mean("sm")) < 1e-6
    assert abs(float(wfm.result()) - mean("wfm")) < 1e-6 and abs(float(em.result()) - mean("em_curve").mean()) < 1e-6
    assert abs(float(fm.result()) - mean("fm_curve").mean()) < 1e-6 and abs(float(em.adaptive_result()) - mean("em_adp")) < 1e-6
    assert abs(float(fm.adaptive_result()) - mean("fm_adp")) < 1e-6
    assert np.allclose(fm.precision_curve().numpy(), mean("precision"), atol=1e-6) and np.allclose(fm.recall_curve().numpy(), mean("recall"), atol=1e-6)
    assert np.allclose(em.curve_result().numpy(), mean("em_curve"), atol=1e-6) and np.allclose(fm.curve_result().numpy(), mean("fm_curve"), atol=1e-6)
    st.reset_state()
    assert float(sm.result()) == 0.0 and int(st.count) == 0


@pytest.mark.parametrize("case", ["odd_37x53_saliency", "odd_37x53_uniform", "2x64x96_uint8_normalize"])
def test_fused_route_equals_composed_route(cuda, monkeypatch, case):
    from iseg_amd.metrics.sod import SodMetricSet

    pred, gt, normalize = CASES[case]()
    _assert_threshold_clear(_as_float(pred, gt, normalize)[0])
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("ISEG_SODMETRICS_FUSED", route)
        st = SodMetricSet(_metrics())
        st.update_state(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), normalize=normalize)
        out[route] = st.state.cpu().numpy()
        assert int(st.count) == pred.shape[0]
    B = pred.shape[0]
    _gap("fused vs composed, counts-only entries", out["1"][[2, 3] + list(range(5, 1032))] / B, out["0"][[2, 3] + list(range(5, 1032))] / B, INT_BOUND)
    _gap("fused vs composed, MAE / S / weighted F", out["1"][[0, 1, 4]] / B, out["0"][[0, 1, 4]] / B, FLOAT_BOUND)


def test_accumulated_updates_equal_the_batched_call(cuda):
    from iseg_amd.metrics.sod import SodMetricSet

    p, g = saliency(6, 40, 56, 12)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    a, b = SodMetricSet(_metrics()), SodMetricSet(_metrics())
    a.update_state(P, G)
    b.update_state(P[0], G[0])      # one 2-D image, as the reference takes it
    b.update_state(P[1:4], G[1:4])
    b.update_state(P[4:], G[4:])
    assert torch.equal(a.state, b.state) and int(a.count) == int(b.count) == 6
    # and at a size whose images are split over many workgroups: an image's partial sums must not depend on how many images share the call
    p, g = saliency(3, 512, 300, 16)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    a, b = SodMetricSet(_metrics()), SodMetricSet(_metrics())
    a.update_state(P, G)
    for k in range(3):
        b.update_state(P[k], G[k])
    assert torch.equal(a.state, b.state) and int(a.count) == int(b.count) == 3


def test_identical_updates_give_bit_identical_state(cuda):
    from iseg_amd.metrics.sod import SodMetricSet

    p, g = saliency(3, 130, 200, 13)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    runs = []
    for _ in range(3):
        st = SodMetricSet(_metrics())
        st.update_state(P, G)
        runs.append(st.state.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


def test_metric_set_launches_the_shared_passes_once(cuda):
    from iseg_amd import kernels as K
    from iseg_amd.metrics.sod import SodMetricSet

    p, g = saliency(2, 32, 48, 14)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    st = SodMetricSet(_metrics())
    n0 = K.SOD_CALLS[0]
    st.update_state(P, G)
    assert K.SOD_CALLS[0] - n0 == 1
    alone = _metrics()
    n0 = K.SOD_CALLS[0]
    for m in alone:
        m.update_state(P, G)
    assert K.SOD_CALLS[0] - n0 == 5
    for m, s in zip(alone, st.metrics):
        assert torch.equal(m.result(), s.result())
    with pytest.raises(RuntimeError):      # a member updated on its own would count the images for every member
        st.metrics[2].update_state(P, G)


def test_update_state_replays_from_a_captured_graph_without_a_host_read(cuda):
    """a capture fails on any host synchronisation, so a successful capture is the proof; the replays then follow the eager updates bit for bit"""
    from iseg_amd.metrics.sod import SodMetricSet

    p, g = saliency(2, 64, 80, 15)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    eager = SodMetricSet(_metrics())
    for _ in range(3):
        eager.update_state(P, G)
    st = SodMetricSet(_metrics())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st.update_state(P, G)      # warm-up on the capture stream: the workspace may not grow under capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    st.reset_state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        st.update_state(P, G)
    st.reset_state()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(st.count) == 6 and torch.equal(st.state, eager.state)


def test_refusals(cuda):
    from iseg_amd import kernels as K

    P, G = torch.rand(1, 8, 8).cuda(), torch.zeros(1, 8, 8, dtype=torch.bool).cuda()
    with pytest.raises(TypeError):
        K.sod_metrics(P, G, normalize=True)      # normalize takes uint8
    with pytest.raises(ValueError):
        K.sod_metrics(P, G[:, :4])
