"""FmeasureV2 through the HIP kernel (csrc/sod_fmv2.hip), by the C ABI wrapper and by the classes, against the restatement
tests/fmeasurev2_ref.py.

Integers (histograms, foreground count, adaptive and binary counts) must be bit-exact.  Each case asserts on the CPU, before anything is compared,
two conditions on the INPUTS: no pixel lies within 4 fp32 ulps of the adaptive threshold (the threshold is an fp32 rounding of a mean, and the
kernel's fixed-order fp64 mean may differ from NumPy's pairwise one in the last bit), and no pixel's bin is decided by the rounding of the fp32
product p * 255.0f (its integer part equals that of the exact product).  No pixel or image is ever left out of a comparison.

Every score is computed from identical integers by a few fp64 operations on both sides, only their order (and FMA contraction) differs:
INT_BOUND = 1e-9 absolute, the bound tests/test_sod_metrics_gpu.py uses for such quantities.
"""
import functools

import numpy as np
import pytest
import torch

from tests import fmeasurev2_ref as R

pytestmark = pytest.mark.gpu

INT_BOUND = 1e-9
WORST = {}
ALL_MODES = 7


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


def constant_grey(B, H, W, seed, level=51):
    """max = min: prepare_data skips mapminmax and every pixel is level / 255"""
    rng = np.random.default_rng(seed)
    return np.full((B, H, W), level, np.uint8), rng.integers(0, 256, (B, H, W)).astype(np.uint8)


CASES = {
    "odd_37x53_saliency": lambda: saliency(1, 37, 53, 1) + (False,),
    "odd_37x53_uniform": lambda: uniform(1, 37, 53, 2) + (False,),
    "4x128x160_saliency": lambda: saliency(4, 128, 160, 3) + (False,),
    "3x61x67_uint8_normalize": lambda: grey(3, 61, 67, 4) + (True,),
    "2x64x96_uint8_normalize": lambda: grey(2, 64, 96, 5) + (True,),
    "2x33x48_uint8_constant": lambda: constant_grey(2, 33, 48, 8) + (True,),
    "3x512x300_saliency": lambda: saliency(3, 512, 300, 16) + (False,),
    "1x1024x1024_saliency": lambda: saliency(1, 1024, 1024, 7) + (False,),
}
SMALL = ["odd_37x53_saliency", "odd_37x53_uniform", "2x64x96_uint8_normalize"]


def _as_float(pred, gt, normalize):
    if not normalize:
        return pred, gt
    out = [R.S.prepare_data(pred[b], gt[b]) for b in range(pred.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _assert_input_condition(p):
    for b in range(p.shape[0]):
        thr = R.S.adaptive_threshold(p[b])
        gap = np.abs(p[b].view(np.int32).astype(np.int64) - int(thr.view(np.int32)))
        assert int(gap.min()) > 4, f"input condition: a pixel of image {b} lies within 4 ulps of the adaptive threshold {thr}"
        prod32 = (p[b] * np.float32(255.0)).astype(np.int64)
        exact = np.floor(p[b].astype(np.float64) * 255.0).astype(np.int64)      # an fp32 value times 255 is exact in fp64
        assert np.array_equal(prod32, exact), f"input condition: the rounding of p * 255.0f decides the bin of a pixel of image {b}"


@functools.lru_cache(maxsize=None)
def _case(name):
    """(pred, gt, normalize, the restatement of every image), computed once and shared; nothing in it is written to"""
    pred, gt, normalize = CASES[name]()
    p, g = _as_float(pred, gt, normalize)
    _assert_input_condition(p)
    return pred, gt, normalize, [R.all_handlers(p[b], g[b]) for b in range(p.shape[0])]


def _table(modes=ALL_MODES, beta=0.3):
    return [(k, modes, beta) for k in range(10)]


def _gap(name, got, want, bound):
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))))
    WORST[name] = max(WORST.get(name, 0.0), err)
    assert np.all(np.isfinite(got)) and err <= bound, (name, err, bound)


def _call(cuda, pred, gt, normalize, table, **kw):
    from iseg_amd import kernels as K

    state = torch.zeros(len(table), K.SODV2_HANDLER_DOUBLES, dtype=torch.float64, device=cuda)
    count = torch.zeros(1, dtype=torch.int64, device=cuda)
    ints, per = K.sod_fmv2(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), table, normalize=normalize, state=state, count=count, **kw)
    return state, count, ints, per


@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_restatement(cuda, case):
    """all ten kinds x all three modes in one call"""
    pred, gt, normalize, want = _case(case)
    state, count, ints, per = _call(cuda, pred, gt, normalize, _table(), want_ints=True, want_per_image=True)
    ints, per = ints.cpu().numpy(), per.cpu().numpy()
    B = pred.shape[0]
    assert int(count) == B and per.shape == (B, 10, 264) and ints.shape == (B, 520)
    total = np.zeros((10, 264))
    for b in range(B):
        w = want[b]
        wi = w["ints"]
        assert np.array_equal(ints[b, :256], wi["hist_fg"]) and np.array_equal(ints[b, 256:512], wi["hist_bg"]), "histograms"
        assert ints[b, 512] == wi["nfg"] and (ints[b, 513], ints[b, 514]) == (wi["nge"], wi["ngefg"]), "foreground and adaptive counts"
        assert (ints[b, 515], ints[b, 516]) == (wi["n05"], wi["n05fg"]), "binary counts"
        assert abs(int(ints[b, 517]) - int(wi["thr"].view(np.int32))) <= 1, "adaptive threshold"
        assert not ints[b, 518:].any()
        for k, kind in enumerate(R.KINDS):
            _gap(kind, per[b, k, :256], w[kind]["dynamic"], INT_BOUND)
            _gap(kind, per[b, k, 256], w[kind]["adaptive"], INT_BOUND)
            _gap(kind, per[b, k, 257], w[kind]["binary"], INT_BOUND)
            assert tuple(per[b, k, 258:262]) == w["binary_counts"] and not per[b, k, 262:].any()
        total += per[b]
    # the running state is the images added in order
    assert np.array_equal(state.cpu().numpy(), total)
    print(case, "worst gap per kind so far:", {k: f"{v:.2e}" for k, v in WORST.items()})


NAMES = dict(TFIOUHandler="iou", TFSpecificityHandler="specificity", TFDICEHandler="dice", TFOverallAccuracyHandler="overall_accuracy",
             TFKappaHandler="kappa", TFPrecisionHandler="precision", TFRecallHandler="recall", TFFPRHandler="fpr", TFBERHandler="ber",
             TFFmeasureHandler="fmeasure")


def _handlers(dynamic=True, adaptive=True, binary=True, sample_based=True):
    import iseg_amd.metrics.sod as sod

    return {name: getattr(sod, cls)(dynamic, adaptive, with_binary=binary, sample_based=sample_based) for cls, name in NAMES.items()}


@functools.lru_cache(maxsize=None)
def _five():
    p, g = saliency(5, 45, 52, 11)
    g[1] = False
    g[2] = True
    _assert_input_condition(p)
    return p, g, [R.all_handlers(p[b], g[b]) for b in range(5)]


def test_classes_against_the_restatement_and_degenerate_gts(cuda):
    """through the classes: an all-background and an all-foreground gt among ordinary images; result() is fp32, as the reference's safe_divide"""
    from iseg_amd.metrics.sod import TFFmeasureV2

    p, g, want = _five()
    ev = TFFmeasureV2(_handlers())
    ev.update_state(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), normalize=False)
    res = ev.result()
    assert list(res) == list(NAMES.values())
    for kind in R.KINDS:
        r = res[kind]
        assert list(r) == ["dynamic", "adaptive", "binary"] and r["dynamic"].shape == (256,) and r["dynamic"].dtype == torch.float32
        _gap(kind + " (classes)", r["dynamic"].numpy(), np.mean([w[kind]["dynamic"] for w in want], axis=0), 1e-6)
        _gap(kind + " (classes)", float(r["adaptive"]), np.mean([w[kind]["adaptive"] for w in want]), 1e-6)
        _gap(kind + " (classes)", float(r["binary"]), np.mean([w[kind]["binary"] for w in want]), 1e-6)
    ev.reset_state()
    assert int(ev.count) == 0 and not ev.state.any() and float(ev.result()["dice"]["adaptive"]) == 0.0


@functools.lru_cache(maxsize=None)
def _two_batches():
    """two updates of different images and image sizes (with one size the pooled overall accuracy IS the mean of the per-image ones)"""
    out = []
    for B, H, W, seed in ((1, 45, 52, 21), (2, 24, 40, 22)):
        p, g = saliency(B, H, W, seed)
        _assert_input_condition(p)
        out.append((p, g, [R.all_handlers(p[b], g[b]) for b in range(B)]))
    return out


def test_dataset_based_binary_mode(cuda):
    """sample_based=False: binary is compute_metric of the counts summed over two updates, not the mean of the per-image scores"""
    from iseg_amd.metrics.sod import TFFmeasureV2

    ds, sb = TFFmeasureV2(_handlers(sample_based=False)), TFFmeasureV2(_handlers())
    used = []
    for p, g, want in _two_batches():
        for ev in (ds, sb):
            ev.update_state(torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda(), normalize=False)
        used += want
    tot = [sum(w["binary_counts"][j] for w in used) for j in range(4)]
    dres, sres = ds.result(), sb.result()
    for kind in R.KINDS:
        pooled, mean = float(R.compute_metric(kind, *tot)), float(np.mean([w[kind]["binary"] for w in used]))
        _gap(kind + " (dataset)", float(dres[kind]["binary"]), pooled, 1e-6)
        _gap(kind + " (classes)", float(sres[kind]["binary"]), mean, 1e-6)
        # the two modes differ on this data by more than ten times the 1e-6 each is checked to, so the test can tell them apart
        assert abs(pooled - mean) > 1e-5 and abs(float(dres[kind]["binary"]) - float(sres[kind]["binary"])) > 1e-5, kind
        assert torch.equal(dres[kind]["dynamic"], sres[kind]["dynamic"])


@pytest.mark.parametrize("case", SMALL)
def test_fused_route_equals_composed_route(cuda, monkeypatch, case):
    from iseg_amd.metrics.sod import TFFmeasureV2

    pred, gt, normalize, _ = _case(case)
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("ISEG_SODFMV2_FUSED", route)
        ev = TFFmeasureV2(_handlers())
        ev.update_state(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), normalize=normalize)
        out[route] = ev.state.cpu().numpy()
        assert int(ev.count) == pred.shape[0]
    _gap("fused vs composed", out["1"] / pred.shape[0], out["0"] / pred.shape[0], INT_BOUND)


def test_accumulated_updates_equal_the_batched_call(cuda):
    from iseg_amd.metrics.sod import TFFmeasureV2

    p, g = saliency(6, 40, 56, 12)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    a, b = TFFmeasureV2(_handlers()), TFFmeasureV2(_handlers())
    a.update_state(P, G, normalize=False)
    b.update_state(P[0], G[0], normalize=False)      # one 2-D image, as the reference takes it
    b.update_state(P[1:4], G[1:4], normalize=False)
    b.update_state(P[4:], G[4:], normalize=False)
    assert torch.equal(a.state, b.state) and int(a.count) == int(b.count) == 6
    # and at a size whose images are split over many workgroups: an image's partial sums must not depend on how many images share the call
    pred, gt, _, _ = _case("3x512x300_saliency")
    P, G = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    a, b = TFFmeasureV2(_handlers()), TFFmeasureV2(_handlers())
    a.update_state(P, G, normalize=False)
    for k in range(3):
        b.update_state(P[k], G[k], normalize=False)
    assert torch.equal(a.state, b.state) and int(a.count) == int(b.count) == 3
    # uint8: the same through the one-pass route
    u, g8 = grey(3, 61, 67, 4)
    U, G8 = torch.from_numpy(u).cuda(), torch.from_numpy(g8).cuda()
    a, b = TFFmeasureV2(_handlers()), TFFmeasureV2(_handlers())
    a.update_state(U, G8)
    for k in range(3):
        b.update_state(U[k], G8[k])
    assert torch.equal(a.state, b.state) and int(a.count) == int(b.count) == 3


def test_identical_updates_give_bit_identical_state(cuda):
    from iseg_amd.metrics.sod import TFFmeasureV2

    p, g = saliency(3, 130, 200, 13)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    runs = []
    for _ in range(3):
        ev = TFFmeasureV2(_handlers())
        ev.update_state(P, G, normalize=False)
        runs.append(ev.state.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]) and bool(runs[0].any())


def test_evaluator_launches_once_for_all_handlers(cuda):
    from iseg_amd import kernels as K
    from iseg_amd.metrics.sod import TFFmeasureV2

    p, g = saliency(2, 32, 48, 14)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    ev = TFFmeasureV2(_handlers())
    n0 = K.SODV2_CALLS[0]
    ev.update_state(P, G, normalize=False)
    assert K.SODV2_CALLS[0] - n0 == 1
    one = TFFmeasureV2({"iou": _handlers()["iou"]})
    n0 = K.SODV2_CALLS[0]
    one.update_state(P, G, normalize=False)
    assert K.SODV2_CALLS[0] - n0 == 1
    alone = _handlers()
    n0 = K.SODV2_CALLS[0]
    for h in alone.values():
        h.update_state(P, G, normalize=False)
    assert K.SODV2_CALLS[0] - n0 == 10
    res = ev.result()
    for name, h in alone.items():
        for mode, v in h.result().items():
            assert torch.equal(v, res[name][mode]), (name, mode)
    with pytest.raises(RuntimeError):      # a member updated on its own would count the images for every member
        ev._metric_handlers["dice"].update_state(P, G, normalize=False)


def test_update_state_replays_from_a_captured_graph_without_a_host_read(cuda):
    """a capture fails on any host synchronisation or host-to-device copy, so a successful capture is the proof; the replays then follow the
    eager updates bit for bit"""
    from iseg_amd.metrics.sod import TFFmeasureV2

    p, g = saliency(2, 64, 80, 15)
    P, G = torch.from_numpy(p).cuda(), torch.from_numpy(g).cuda()
    eager = TFFmeasureV2(_handlers())
    for _ in range(3):
        eager.update_state(P, G, normalize=False)
    ev = TFFmeasureV2(_handlers())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev.update_state(P, G, normalize=False)      # warm-up on the capture stream: the workspace may not grow under capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ev.reset_state()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ev.update_state(P, G, normalize=False)
    ev.reset_state()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(ev.count) == 6 and torch.equal(ev.state, eager.state)


@pytest.mark.parametrize("case", ["odd_37x53_saliency", "4x128x160_saliency"])
def test_adaptive_pass_does_not_perturb_the_rest(cuda, case):
    """the second pass runs only when some handler records the adaptive mode: dynamic and binary slots are bit-identical with and without it"""
    pred, gt, normalize, _ = _case(case)
    D, A, Bn = 1, 2, 4
    s_d, _, i_d, _ = _call(cuda, pred, gt, normalize, _table(D), want_ints=True)
    s_da, _, i_da, _ = _call(cuda, pred, gt, normalize, _table(D | A), want_ints=True)
    s_db, _, _, _ = _call(cuda, pred, gt, normalize, _table(D | Bn))
    s_all, _, i_all, _ = _call(cuda, pred, gt, normalize, _table(D | A | Bn), want_ints=True)
    assert torch.equal(s_d[:, :256], s_da[:, :256]) and torch.equal(s_d[:, :256], s_all[:, :256]) and bool(s_d[:, :256].any())
    assert not s_d[:, 256:].any() and not s_da[:, 257:].any() and bool(s_da[:, 256].any())
    assert torch.equal(s_db[:, 257:], s_all[:, 257:]) and torch.equal(s_da[:, 256], s_all[:, 256]) and not s_db[:, 256].any()
    assert torch.equal(i_d[:, :513], i_da[:, :513]) and torch.equal(i_d[:, 515:517], i_da[:, 515:517]) and torch.equal(i_da, i_all)
    assert not i_d[:, 513:515].any() and not i_d[:, 517].any()      # an fp32 prediction without the adaptive mode: no threshold, no second pass


def test_refusals(cuda):
    from iseg_amd import _hip
    from iseg_amd import kernels as K

    P, G = torch.rand(1, 8, 8).cuda(), torch.zeros(1, 8, 8, dtype=torch.bool).cuda()
    with pytest.raises(TypeError):
        K.sod_fmv2(P, G, _table(), normalize=True)      # normalize takes uint8
    with pytest.raises(TypeError):
        K.sod_fmv2((P * 255).to(torch.uint8), G, _table())      # and only normalize does
    with pytest.raises(ValueError):
        K.sod_fmv2(P, G[:, :4], _table())
    with pytest.raises(_hip.HipCallError, match="0 handlers"):
        K.sod_fmv2(P, G, [])
    with pytest.raises(_hip.HipCallError, match="33 handlers"):
        K.sod_fmv2(P, G, [(0, 1, 0.3)] * 33)
    with pytest.raises(_hip.HipCallError, match="unknown kind"):
        K.sod_fmv2(P, G, [(0, 1, 0.3), (10, 1, 0.3)])
    with pytest.raises(_hip.HipCallError, match="unknown mode"):
        K.sod_fmv2(P, G, [(0, 8, 0.3)])
    K.sod_fmv2(P, G, [(0, 1, 0.3)] * 32)      # the most one call takes
    torch.cuda.synchronize()
