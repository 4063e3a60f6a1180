"""Confusion matrices through the HIP kernel (csrc/confusion.hip): by the C ABI wrapper kernels.confusion_batched, by metrics/confusion_matrix.py
and by the mean_iou / seg_metric_wrapper functions built on it, against the numpy restatement tests/confusion_ref.py.  The kernel's result is
integers: every comparison is exact (np.array_equal / torch.equal) except the one against a float64 sum, whose bound is the fixed-point rule's.

Q = 4096 elements per workgroup and trip, at most 1024 workgroups per launch (ISEG_CM_SLICE, ISEG_CM_GRID_CAP), fewer where the histogram's
LDS lets a CU hold fewer than four workgroups (256 from C = 144 on, from C = 102 with fp32 weights).  Route boundaries (bins that fit
the 160 KiB of LDS in one band, two, three, four): 32-bit bins C = 202 | 203; 64-bit bins C = 143 | 144, 202 | 203, 246 | 247.  An image whose
length is no multiple of 4 takes the scalar loads, the others the 16-byte ones: the element counts cover both."""
import numpy as np
import pytest
import torch

from tests import confusion_ref as R
from tests import guarded_memory as GM

pytestmark = pytest.mark.gpu

Q, CAP = R.SLICE, R.GRID_CAP
CLASSES = [1, 2, 21, 143, 144, 150, 202, 203, 246, 247, 256]
LENGTHS = [1, 63, 64, 65, Q - 1, Q, Q + 1, 2 * Q + 2052, 3 * Q + 17]      # Q and 2 Q + 2052: 16-byte loads, whole and with a ragged second chunk
MODES = [R.W_NONE, R.W_U8, R.W_F32]
MODE_NAMES = {R.W_NONE: "none", R.W_U8: "u8", R.W_F32: "f32"}


def K():
    from iseg_amd import kernels

    return kernels


def case(B, n, C, mode, seed=0):
    """labels, preds [B, n] int32 in [0, C), weights None / uint8 / float32 (multiples of 1/8 up to +-31, a tenth of them 0)"""
    g = np.random.default_rng([seed, B, n, C, mode])
    lab = g.integers(0, C, (B, n)).astype(np.int32)
    prd = g.integers(0, C, (B, n)).astype(np.int32)
    if mode == R.W_NONE:
        return lab, prd, None
    if mode == R.W_U8:
        return lab, prd, g.integers(0, 256, (B, n)).astype(np.uint8)
    w = (g.integers(-248, 249, (B, n)) / 8.0).astype(np.float32)
    w[g.random((B, n)) < 0.1] = 0
    return lab, prd, w


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def run(cuda, lab, prd, w, C, w_exp=0, **kw):
    cm, counters = K().confusion_batched(dev(lab, cuda), dev(prd, cuda), C, weights=dev(w, cuda), w_exp=w_exp, **kw)
    return cm.cpu().numpy().reshape(lab.shape[0], C, C), counters.cpu().numpy()


def w_exp_of(w):
    return R.weight_exponent(np.abs(w).max()) if w is not None and w.dtype == np.float32 else 0


# ---- shapes, routes, weight modes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES.get)
@pytest.mark.parametrize("C", CLASSES)
def test_matches_the_restatement(cuda, C, mode):
    for B in (1, 3):
        for n in LENGTHS:
            lab, prd, w = case(B, n, C, mode)
            e = w_exp_of(w)
            got, counters = run(cuda, lab, prd, w, C, e)
            want, wc = R.kernel_counts(lab, prd, C, w, e)
            assert np.array_equal(got, want), (C, mode, B, n)
            assert np.array_equal(counters, wc), (C, mode, B, n, counters, wc)


def test_routes_under_test_are_the_dispatchers():
    """one class count on each side of every boundary, and the extremes"""
    bands = {(C, m): R.route(C, m)[0] for C in CLASSES for m in MODES}
    assert [bands[C, R.W_NONE] for C in (202, 203, 256)] == [1, 2, 2] and [bands[C, R.W_U8] for C in (202, 203)] == [1, 2]
    assert [bands[C, R.W_F32] for C in (143, 144, 202, 203, 246, 247, 256)] == [1, 2, 2, 3, 3, 4, 4]
    assert all(R.route(C, m)[2] == "lds" for C in CLASSES for m in MODES)


@pytest.mark.parametrize("C,mode,cap", [(21, R.W_NONE, CAP), (150, R.W_U8, 256), (256, R.W_F32, 256)], ids=["C21-none-1024", "C150-u8-256", "C256-f32-256"])
def test_slice_count_past_the_grid_cap(cuda, C, mode, cap):
    """Q = 4096; the cap is 1024 workgroups while four histograms fit a CU and 256 where one does (C = 150 in 32-bit bins, C = 256 in four
    bands of 64-bit bins).  B = 1 and 2 * cap + 77 slices and 17 elements more: two full trips of the persistent loop and a ragged third"""
    n = (2 * cap + 77) * Q + 17
    gx, gy, slices, trips = R.grid(1, n, C, mode)
    assert R.grid_cap(C, mode) == cap and (gx, gy) == (cap, 1) and slices == 2 * cap + 78 and trips == 3
    assert slices > 2 * gx and slices % gx != 0 and n % Q != 0
    lab, prd, w = case(1, n, C, mode)
    e = w_exp_of(w)
    val = np.ones(n, np.int64) if w is None else np.rint(w[0].astype(np.float64) * 2.0 ** e).astype(np.int64)
    assert w is None or np.array_equal(val * 2.0 ** -e, w[0])      # (exact weights: the integer reference below is the whole story)

    def want(first):
        idx = lab[0, first:].astype(np.int64) * C + prd[0, first:]
        pos = np.bincount(idx, weights=np.maximum(val[first:], 0), minlength=C * C)      # float64 sums of integers below 2^53: exact
        neg = np.bincount(idx, weights=np.maximum(-val[first:], 0), minlength=C * C)
        return (pos.astype(np.int64) - neg.astype(np.int64)).reshape(1, C, C)

    got, counters = run(cuda, lab, prd, w, C, e)
    assert np.array_equal(got, want(0)) and not counters.any()
    # the ragged trip alone: the elements from the first slice of the third trip on
    first = 2 * gx * Q
    got_tail, _ = run(cuda, lab[:, first:], prd[:, first:], None if w is None else w[:, first:], C, e)
    assert np.array_equal(got_tail, want(first))


# ---- contention ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES.get)
def test_every_element_in_one_bin(cuda, mode):
    n, C = 1 << 20, 5
    lab = torch.full((1, n), 3, dtype=torch.int32, device=cuda)
    prd = torch.full((1, n), 1, dtype=torch.int32, device=cuda)
    w, each, e = None, 1, 0
    if mode == R.W_U8:
        w, each = torch.full((1, n), 255, dtype=torch.uint8, device=cuda), 255
    if mode == R.W_F32:
        w, e = torch.full((1, n), 0.75, dtype=torch.float32, device=cuda), R.weight_exponent(0.75)
        each = 3 << (e - 2)
    cm, counters = K().confusion_batched(lab, prd, C, weights=w, w_exp=e)
    want = torch.zeros(1, C, C, dtype=torch.int64)
    want[0, 3, 1] = n * each
    assert torch.equal(cm.cpu(), want) and not counters.any()


def test_u8_weight_255_at_the_private_counter_bound(cuda):
    """n = 2^24 + 5, B = 1: five trips of 1024 workgroups, 20480 elements of weight 255 in ONE 32-bit bin of each; the exact total"""
    n = (1 << 24) + 5
    gx, gy, slices, trips = R.grid(1, n, 2, R.W_U8)
    assert (gx, trips) == (CAP, 5) and trips * Q * 255 < 2 ** 32
    lab = torch.zeros(1, n, dtype=torch.int32, device=cuda)
    w = torch.full((1, n), 255, dtype=torch.uint8, device=cuda)
    cm, counters = K().confusion_batched(lab, lab, 2, weights=w)
    assert cm.cpu().reshape(-1).tolist() == [255 * n, 0, 0, 0] and not counters.any()


# ---- fp32 weights -----------------------------------------------------------------------------------------------------------------------------
def test_f32_second_run_and_permutation_are_bit_identical(cuda):
    lab, prd, w = R.dynamic_range_case(n=3 * Q + 17, C=5, seed=11)
    lab, prd, w = np.repeat(lab, 2, 0), np.repeat(prd, 2, 0), np.repeat(w, 2, 0)
    e = w_exp_of(w)
    a, ca = run(cuda, lab, prd, w, 5, e)
    b, cb = run(cuda, lab, prd, w, 5, e)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)
    g = np.random.default_rng(5)
    perm = np.stack([g.permutation(lab.shape[1]) for _ in range(2)])
    take = lambda x: np.take_along_axis(x, perm, 1)      # noqa: E731
    c, cc = run(cuda, take(lab), take(prd), take(w), 5, e)
    assert np.array_equal(a, c) and np.array_equal(ca, cc)
    want, wc = R.kernel_counts(lab, prd, 5, w, e)
    assert np.array_equal(a, want) and np.array_equal(ca, wc) and wc[5] > 0 and not wc[:5].any()      # (most of these weights are rounded)


def test_f32_plus_and_minus_pairs_cancel_exactly(cuda):
    from iseg_amd.metrics.confusion_matrix import confusion_matrix

    g = np.random.default_rng(2)
    w = (g.standard_normal(5000) * 10.0 ** g.uniform(-6, 3, 5000)).astype(np.float32)
    w = np.concatenate([w, -w])[g.permutation(10000)]
    z = torch.zeros(10000, dtype=torch.int32, device=cuda)
    cm = confusion_matrix(z + 2, z + 1, 4, weights=dev(w, cuda), dtype=torch.float64)
    assert cm.dtype == torch.float64 and tuple(cm.shape) == (4, 4) and not cm.any()


def test_f32_dynamic_range_stays_inside_the_bound(cuda):
    """2^18 elements, C = 5, Gaussian weights times 10^U(-6, 3), against a float64 np.add.at:
    |got - ref64| <= 2^-23 |ref64| + k max|w| 2^-38 per bin (k the bin's element count); and exactly the restated fixed-point sums"""
    from iseg_amd.metrics.confusion_matrix import batch_confusion_matrix

    lab, prd, w = R.dynamic_range_case()
    got = batch_confusion_matrix(dev(lab, cuda), dev(prd, cuda), 5, weights=dev(w, cuda), dtype=torch.float64).cpu().numpy()
    ref, bound = R.fixed_point_bound(lab, prd, 5, w)
    print("worst ratio to the bound", (np.abs(got - ref) / bound).max())
    assert (np.abs(got - ref) <= bound).all()
    assert np.array_equal(got, R.fixed_point_matrix(lab, prd, 5, w)[0])


def test_f32_all_zero_weights(cuda):
    from iseg_amd.metrics.confusion_matrix import confusion_matrix

    lab, prd, _ = case(1, 1000, 7, R.W_NONE)
    assert K().confusion_absmax(torch.zeros(1000, device=cuda)) == 0.0
    cm = confusion_matrix(dev(lab[0], cuda), dev(prd[0], cuda), 7, weights=torch.zeros(1000, device=cuda), dtype=torch.float32)
    assert cm.dtype == torch.float32 and not cm.any()


def test_absmax_is_exact(cuda):
    g = np.random.default_rng(4)
    for n in (1, 5, 4099, 3 * 1024 * 1024 + 7):
        w = (g.standard_normal(n) * 10.0 ** g.uniform(-6, 3, n)).astype(np.float32)
        assert K().confusion_absmax(dev(w, cuda)) == float(np.abs(w).max())
        if n > 4:      # a base that is only 4-byte aligned: the scalar loads
            assert K().confusion_absmax(dev(w, cuda)[1:-1]) == float(np.abs(w[1:-1]).max())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_f32_non_finite_weights_raise(cuda, bad):
    from iseg_amd.metrics.confusion_matrix import batch_confusion_matrix, confusion_matrix

    z = torch.zeros(100, dtype=torch.int32, device=cuda)
    w = torch.ones(100, device=cuda)
    w[37] = bad
    with pytest.raises(ValueError, match="not finite"):
        confusion_matrix(z, z, 2, weights=w, dtype=torch.float32)
    with pytest.raises(ValueError, match="not finite"):
        batch_confusion_matrix(z.reshape(4, 25), z.reshape(4, 25), 2, weights=w.reshape(4, 25), dtype=torch.float32)
    # the raw entry point counts it, skips it and counts the others
    cm, counters = K().confusion_batched(z.reshape(1, -1), z.reshape(1, -1), 2, weights=w.reshape(1, -1))
    assert cm.cpu().reshape(-1).tolist() == [99, 0, 0, 0] and counters.cpu().tolist() == [0, 0, 0, 0, 1, 0, 0, 0]


def test_f32_past_2_24_elements_refuses_and_leaves_cm_untouched(cuda):
    from iseg_amd import _hip

    n = (1 << 24) + 1
    z = torch.zeros(1, n, dtype=torch.int32, device=cuda)
    w = torch.ones(1, n, device=cuda)
    cm = torch.full((1, 2, 2), 77, dtype=torch.int64, device=cuda)
    counters = torch.full((8,), 5, dtype=torch.int64, device=cuda)
    with pytest.raises(_hip.HipCallError, match=r"status -3.*2\^24"):
        K().confusion_batched(z, z, 2, weights=w, cm=cm, counters=counters)
    assert (cm == 77).all() and (counters == 5).all()
    cm2, _ = K().confusion_batched(z, z, 2)      # the same length without weights counts
    assert cm2.cpu().reshape(-1).tolist() == [n, 0, 0, 0]


# ---- accumulate, ignore, rejected elements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES.get)
def test_accumulate_twice_gives_twice_the_matrix(cuda, mode):
    lab, prd, w = case(3, Q + 1, 21, mode)
    e = w_exp_of(w)
    once, _ = run(cuda, lab, prd, w, 21, e)
    cm = torch.zeros(3, 21, 21, dtype=torch.int64, device=cuda)
    counters = torch.zeros(8, dtype=torch.int64, device=cuda)
    for _ in range(2):
        K().confusion_batched(dev(lab, cuda), dev(prd, cuda), 21, weights=dev(w, cuda), w_exp=e, cm=cm, accumulate=True, counters=counters)
    assert np.array_equal(cm.cpu().numpy(), 2 * once) and once.any()
    K().confusion_batched(dev(lab, cuda), dev(prd, cuda), 21, weights=dev(w, cuda), w_exp=e, cm=cm, accumulate=False, counters=counters)
    assert np.array_equal(cm.cpu().numpy(), once)


@pytest.mark.parametrize("ignore", [255, 0, -1])
def test_ignore_label_is_skipped_whatever_its_prediction(cuda, ignore):
    C = 6
    lab, prd, w = case(2, Q + 65, C, R.W_U8, seed=3)
    g = np.random.default_rng(9)
    hit = g.random(lab.shape) < 0.2
    if ignore == 0:
        hit |= lab == 0
    lab[hit] = ignore
    prd[0, np.flatnonzero(hit[0])[:3]] = (-5, C, 1 << 30)      # ignored elements with impossible predictions: NOT rejected
    for weights in (None, w, (w / 4).astype(np.float32)):
        got, counters = run(cuda, lab, prd, weights, C, 2 if weights is not None and weights.dtype == np.float32 else 0, ignore_label=ignore)
        want, wc = R.kernel_counts(lab, prd, C, weights, 2, ignore_label=ignore)
        assert np.array_equal(got, want) and not counters.any() and not wc.any()
        assert got.sum() == (np.ones_like(lab) if weights is None else weights.astype(np.float64) * (4 if weights.dtype == np.float32 else 1))[~hit].sum()


BAD = [("label_negative", 0, -1, None), ("prediction_negative", 1, None, -7), ("label_out_of_bound", 2, 9, None), ("prediction_out_of_bound", 3, None, 1 << 20)]


@pytest.mark.parametrize("name,counter,bad_label,bad_pred", BAD, ids=[b[0] for b in BAD])
def test_one_bad_element_among_valid_ones(cuda, name, counter, bad_label, bad_pred):
    from iseg_amd.metrics.confusion_matrix import batch_confusion_matrix, confusion_matrix

    C = 9
    for mode in MODES:
        lab, prd, w = case(2, Q + 65, C, mode, seed=4)
        at = (1, Q + 3)
        if bad_label is not None:
            lab[at] = bad_label
        if bad_pred is not None:
            prd[at] = bad_pred
        if w is not None:
            w[at] = 3
        e = w_exp_of(w)
        got, counters = run(cuda, lab, prd, w, C, e)
        keep = np.ones(lab.shape, bool)
        keep[at] = False
        want = np.zeros((2, C, C), np.int64)
        val = np.ones(lab.shape, np.int64) if w is None else np.rint(w.astype(np.float64) * 2.0 ** e).astype(np.int64)
        np.add.at(want, (np.broadcast_to(np.arange(2)[:, None], lab.shape)[keep], lab[keep], prd[keep]), val[keep])
        assert counters.tolist() == [int(k == counter) for k in range(8)]
        assert np.array_equal(got, want)      # every valid element is counted, every other bin is as expected
        msg = R.MESSAGES[counter].replace("`", ".")
        with pytest.raises(ValueError, match=msg):
            batch_confusion_matrix(dev(lab, cuda), dev(prd, cuda), C, weights=dev(w, cuda), dtype=torch.float64)
        with pytest.raises(ValueError, match=msg):
            confusion_matrix(dev(lab[1], cuda), dev(prd[1], cuda), C, weights=dev(None if w is None else w[1], cuda), dtype=torch.float64)


# ---- guard bands --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES.get)
@pytest.mark.parametrize("C,B,n", [(1, 1, 1), (21, 3, Q + 1), (21, 2, 2 * Q + 2052), (150, 2, 65), (256, 1, 3 * Q + 17)])
def test_nothing_outside_cm_and_counters_is_written(cuda, C, B, n, mode):
    arena = GM.Arena(cuda, 8 << 20)
    lab, prd, w = case(B, n, C, mode, seed=6)
    e = w_exp_of(w)
    with GM.guarded(arena):
        ops = []
        for a in (lab, prd, w):
            if a is not None:
                t = arena.alloc(a.shape, dev(a, cuda).dtype, "operand")
                t.copy_(dev(a, cuda))
                ops.append(t)
            else:
                ops.append(None)
        cm, counters = K().confusion_batched(ops[0], ops[1], C, weights=ops[2], w_exp=e)      # cm = empty (poison), counters = zeros: both in the arena
        assert arena.offset_of(cm) > 0 and arena.offset_of(counters) > 0 and cm.numel() == B * C * C and counters.numel() == 8
        arena.check()
        want, wc = R.kernel_counts(lab, prd, C, w, e)
        assert np.array_equal(cm.cpu().numpy(), want) and np.array_equal(counters.cpu().numpy(), wc)
        assert counters[6:].tolist() == [0, 0]


# ---- relations between the public functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES.get)
def test_batched_sum_flat_and_single_image_agree(cuda, mode):
    from iseg_amd.metrics.confusion_matrix import batch_confusion_matrix, confusion_matrix
    from iseg_amd.metrics.mean_iou import get_batch_class_confusion_matrix, get_class_confusion_matrix

    C = 21
    lab, prd, w = case(3, 37 * 53, C, mode, seed=8)
    shape = (3, 37, 53)
    L, P, W = dev(lab, cuda).reshape(shape), dev(prd, cuda).reshape(shape), None if w is None else dev(w, cuda).reshape(shape)
    dtype = torch.float64 if mode == R.W_F32 else torch.int32
    batched = batch_confusion_matrix(L, P, C, weights=W, dtype=dtype)
    assert tuple(batched.shape) == (3, C, C) and batched.dtype == dtype
    flat = confusion_matrix(L.reshape(-1), P.reshape(-1), C, weights=None if W is None else W.reshape(-1), dtype=dtype)
    assert torch.equal(batched.sum(0).to(dtype), flat)      # (one exponent for the whole call: the fixed-point sums add exactly)
    ref = R.batch_confusion_matrix(lab, prd, C, w, np.float64 if mode == R.W_F32 else np.int32)
    assert np.array_equal(batched.cpu().numpy(), ref)      # weights are multiples of 1/8: the float64 sums are exact too
    assert np.array_equal(flat.cpu().numpy(), R.confusion_matrix(lab.reshape(-1), prd.reshape(-1), C, None if w is None else w.reshape(-1), ref.dtype))
    for b in range(3):
        one = batch_confusion_matrix(L[b:b + 1], P[b:b + 1], C, weights=None if W is None else W[b:b + 1], dtype=dtype)
        assert torch.equal(one[0], batched[b])
    # the mean_iou spellings (default dtype float32) and num_classes = None
    assert torch.equal(get_class_confusion_matrix(L, P, C, W).double(), flat.double())
    assert torch.equal(get_batch_class_confusion_matrix(L, P, C, W).double(), batched.double())
    auto = confusion_matrix(L.reshape(-1), P.reshape(-1), weights=None if W is None else W.reshape(-1), dtype=dtype)
    assert torch.equal(auto, flat) and tuple(auto.shape) == (int(max(lab.max(), prd.max())) + 1,) * 2
    # truncation of float inputs (tf.cast) and a squeezable last dimension
    assert torch.equal(confusion_matrix(L.reshape(-1).float() + 0.9, P.reshape(-1, 1), C, weights=None if W is None else W.reshape(-1), dtype=dtype), flat)


def test_reference_docstring_example_on_the_device(cuda):
    from iseg_amd.metrics.confusion_matrix import confusion_matrix

    got = confusion_matrix(torch.tensor([1, 2, 4], device=cuda), torch.tensor([2, 2, 4], device=cuda))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), R.confusion_matrix([1, 2, 4], [2, 2, 4]))
    frac = confusion_matrix(torch.tensor([1, 1, 1], device=cuda), torch.tensor([0, 0, 0], device=cuda), 2,
                            weights=torch.tensor([0.75, 0.75, 1.25], device=cuda))      # integer dtype: truncated after the sum (2.75 -> 2)
    assert frac.cpu().tolist() == [[0, 0], [2, 0]]


def _logits_case(cuda, C, ignore):
    g = torch.Generator().manual_seed(C + ignore)
    z = torch.randn(2, 12, 9, C, generator=g).to(cuda)
    y = torch.randint(0 if ignore else 1, C + (0 if ignore else 1), (2, 24, 18), generator=g, dtype=torch.int32)
    y[torch.rand(y.shape, generator=g) < 0.15] = ignore
    return z, y.to(cuda)


@pytest.mark.parametrize("ignore", [255, 0])
@pytest.mark.parametrize("weights", ["float32_mask", "bool", "int32"])
def test_update_state_equals_update_from_logits(cuda, ignore, weights):
    from iseg_amd.metrics.mean_iou import MeanIOU
    from iseg_amd.metrics.seg_metric_wrapper import SegMetricWrapper, process_seg_metric_inputs

    C = 7
    z, y = _logits_case(cuda, C, ignore)
    a = MeanIOU(C)
    SegMetricWrapper(a, num_class=C, ignore_label=ignore).update_state(y, z)
    b = MeanIOU(C)
    yt, yp, mask = process_seg_metric_inputs(y, z, num_class=C, ignore_label=ignore)
    assert mask.dtype == torch.float32 and yt.dtype == torch.int32 and yp.dtype == torch.int32
    w = {"float32_mask": mask, "bool": mask.bool(), "int32": mask.to(torch.int32)}[weights]
    for _ in range(2):
        b.update_state(yt, yp, w)
    assert b.total_cm.dtype == torch.int64 and tuple(b.total_cm.shape) == (C * C,)
    assert torch.equal(b.total_cm, 2 * a.total_cm) and int(a.total_cm.sum()) == int(mask.sum())
    assert torch.equal(a.local_result(), b.local_result())
    # without weights every element counts: the ignored ones sit in row 0, where set_ignore_label_to_zero put them
    c = MeanIOU(C)
    c.update_state(yt, yp)
    assert int(c.total_cm.sum()) == yt.numel()


def test_update_state_refuses_fractional_weights_and_keeps_its_counts(cuda):
    from iseg_amd.metrics.mean_iou import MeanIOU

    m = MeanIOU(4)
    y = torch.tensor([0, 1, 2, 3, 3], dtype=torch.int32, device=cuda)
    m.update_state(y, y, torch.tensor([1.0, 2.0, 0.0, 3.0, 1.0], device=cuda))
    before = m.total_cm.clone()
    assert before.reshape(4, 4).diagonal().tolist() == [1, 2, 0, 4]
    with pytest.raises(ValueError, match="get_class_confusion_matrix"):
        m.update_state(y, y, torch.tensor([1.0, 0.5, 1.0, 2.5, 1.0], device=cuda))
    assert torch.equal(m.total_cm, before)
    with pytest.raises(ValueError, match=".labels. out of bound"):
        m.update_state(y + 1, y)      # (its three valid elements are counted, below the diagonal)
    m.update_state(y, y, torch.tensor([2, 2, 2, 2, 2], device=cuda))      # int64 weights
    assert (m.total_cm - before).reshape(4, 4).diagonal().tolist() == [2, 2, 2, 4]
    assert (m.total_cm - before).reshape(4, 4).sum().item() == 10 + 3


# ---- process_seg_metric_inputs ------------------------------------------------------------------------------------------------------------------
def _process_restated(y_true, y_pred, num_class, ignore_label, use_class_prob_as_pred, flatten_outputs, set_ignore_label_to_zero):
    """metrics/seg_metric_wrapper.py:22-68 in torch on the host"""
    from oracle import tf_ops as O

    y_true = y_true.to(torch.int32)
    if y_pred.dim() == 4:
        if y_true.dim() == 3:
            y_true = y_true.unsqueeze(-1)
        y_true = O.resize_nearest(y_true, tuple(y_pred.shape[1:3]))
    if use_class_prob_as_pred:
        if flatten_outputs:
            y_pred = y_pred.reshape(-1, num_class)
        y_pred = torch.argmax(y_pred, dim=-1)
    elif flatten_outputs:
        y_pred = y_pred.reshape(-1)
    y_pred = y_pred.to(torch.int32)
    if flatten_outputs:
        y_true = y_true.reshape(-1)
    mask = y_true != ignore_label
    if ignore_label == 0:
        y_true = y_true - 1
    if set_ignore_label_to_zero:
        y_true = torch.where(mask, y_true, torch.zeros_like(y_true))
    return y_true, y_pred, mask.to(torch.float32)


@pytest.mark.parametrize("ignore", [255, 0])
@pytest.mark.parametrize("as_prob,flatten,to_zero", [(True, True, True), (True, False, True), (True, True, False), (False, True, True), (False, False, False)])
def test_process_seg_metric_inputs(cuda, ignore, as_prob, flatten, to_zero):
    from iseg_amd.metrics.seg_metric_wrapper import process_seg_metric_inputs

    C = 7
    z, y = _logits_case(cuda, C, ignore)      # labels at 24 x 18, logits at 12 x 9: the label map is resized
    pred = z if as_prob else torch.argmax(z, -1).to(torch.int32).unsqueeze(-1)      # a [N, H, W, 1] class map is resized against, too
    got = process_seg_metric_inputs(y, pred, num_class=C, ignore_label=ignore, use_class_prob_as_pred=as_prob, flatten_outputs=flatten,
                                    set_ignore_label_to_zero=to_zero)
    want = _process_restated(y.cpu(), pred.cpu(), C, ignore, as_prob, flatten, to_zero)
    for g, w, name in zip(got, want, ("y_true", "y_pred", "not_ignore_mask")):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), name
    same = process_seg_metric_inputs(y[:, ::2, ::2].contiguous(), pred, num_class=C, ignore_label=ignore,
                                     use_class_prob_as_pred=as_prob, flatten_outputs=flatten, set_ignore_label_to_zero=to_zero)      # already at 12 x 9
    assert tuple(same[0].shape) == tuple(got[0].shape)
