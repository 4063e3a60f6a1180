"""numpy restatement (np.add.at) of metrics/confusion_matrix.py of the reference -- confusion_matrix (:65-143) and batch_confusion_matrix
(:146-231) -- and of the fixed-point path of csrc/confusion.hip (include/iseg_hip.h, iseg_confusion_batched).  Test-only, no torch."""
import math

import numpy as np

MESSAGES = ("`labels` contains negative values", "`predictions` contains negative values", "`labels` out of bound", "`predictions` out of bound")
W_NONE, W_U8, W_F32 = 0, 1, 2
SLICE, GRID_CAP, F32_MAX_N = 4096, 1024, 1 << 24      # ISEG_CM_SLICE, ISEG_CM_GRID_CAP, ISEG_CM_F32_MAX_N


def remove_squeezable_dimensions(labels, predictions, expected_rank_diff=0):
    labels, predictions = np.asarray(labels), np.asarray(predictions)
    d = predictions.ndim - labels.ndim
    if d == expected_rank_diff + 1 and predictions.shape[-1] == 1:
        predictions = predictions[..., 0]
    elif d == expected_rank_diff - 1 and labels.shape[-1] == 1:
        labels = labels[..., 0]
    return labels, predictions


def _checked(labels, predictions, num_classes):
    labels, predictions = np.asarray(labels).astype(np.int32), np.asarray(predictions).astype(np.int32)      # tf.cast: truncation
    if (labels < 0).any():
        raise ValueError(MESSAGES[0])
    if (predictions < 0).any():
        raise ValueError(MESSAGES[1])
    if num_classes is None:
        num_classes = int(max(labels.max(), predictions.max())) + 1
    else:
        if (labels >= num_classes).any():
            raise ValueError(MESSAGES[2])
        if (predictions >= num_classes).any():
            raise ValueError(MESSAGES[3])
    return labels, predictions, int(num_classes)


def confusion_matrix(labels, predictions, num_classes=None, weights=None, dtype=np.int32):
    """tf.scatter_nd(stack([labels, predictions], 1), weights cast to dtype (or ones), [n, n])"""
    labels, predictions = remove_squeezable_dimensions(labels, predictions)
    if labels.ndim != 1 or labels.shape != predictions.shape:
        raise ValueError("shapes")
    labels, predictions, n = _checked(labels, predictions, num_classes)
    values = np.ones(labels.shape, dtype) if weights is None else np.asarray(weights).astype(dtype)
    if values.shape != predictions.shape:
        raise ValueError("weights shape")
    cm = np.zeros((n, n), dtype)
    np.add.at(cm, (labels, predictions), values)
    return cm


def batch_confusion_matrix(labels, predictions, num_classes=None, weights=None, dtype=np.int32):
    labels, predictions = remove_squeezable_dimensions(labels, predictions)
    if labels.shape != predictions.shape or labels.ndim < 1:
        raise ValueError("shapes")
    labels, predictions, n = _checked(labels, predictions, num_classes)
    B = labels.shape[0]
    labels, predictions = labels.reshape(B, -1), predictions.reshape(B, -1)
    values = np.ones(labels.shape, dtype) if weights is None else np.asarray(weights).astype(dtype).reshape(B, -1)
    cm = np.zeros((B, n, n), dtype)
    b = np.broadcast_to(np.arange(B)[:, None], labels.shape)
    np.add.at(cm, (b, labels, predictions), values)
    return cm


# ---- the fixed-point path --------------------------------------------------------------------------------------------------------------------
def weight_exponent(max_abs):
    """38 - ex with max_abs = m * 2^ex, m in [0.5, 1); 0 for 0"""
    max_abs = float(max_abs)
    return 38 - math.frexp(max_abs)[1] if max_abs else 0


def kernel_counts(labels, preds, C, weights=None, w_exp=0, ignore_label=None):
    """iseg_confusion_batched restated: labels, preds [B, n] integers; weights None, uint8 / bool (W_U8) or float32 (W_F32).
    -> (cm [B, C, C] int64, counters [8] int64)"""
    labels, preds = np.asarray(labels).astype(np.int64), np.asarray(preds).astype(np.int64)
    B, n = labels.shape
    counters = np.zeros(8, np.int64)
    live = np.ones(labels.shape, bool) if ignore_label is None else labels != ignore_label
    bad = np.zeros(labels.shape, bool)
    frac = np.zeros(labels.shape, bool)
    if weights is None:
        val = np.ones(labels.shape, np.int64)
    else:
        weights = np.asarray(weights)
        if weights.dtype in (np.uint8, np.bool_):
            val = weights.astype(np.int64)
        else:
            assert weights.dtype == np.float32
            with np.errstate(invalid="ignore", over="ignore"):
                v = weights.astype(np.float64) * math.ldexp(1.0, w_exp)
                out = ~(np.abs(v) < 2.0 ** 39)
                r = np.rint(np.where(out, 0.0, v))      # to nearest even
            val = r.astype(np.int64)
            frac = (r != v) & ~out
            counters[4] = (out & live).sum()
            bad |= out
    for k, cond in enumerate((labels < 0, preds < 0, labels >= C, preds >= C)):
        counters[k] = (cond & live).sum()
        bad |= cond
    keep = live & ~bad
    counters[5] = (frac & keep).sum()
    cm = np.zeros((B, C, C), np.int64)
    b = np.broadcast_to(np.arange(B)[:, None], labels.shape)
    np.add.at(cm, (b[keep], labels[keep], preds[keep]), val[keep])
    return cm, counters


def fixed_point_matrix(labels, preds, C, weights):
    """what the public functions return for float32 weights, as float64: ldexp(kernel_counts, -w_exp) with the exponent from max |w|"""
    weights = np.asarray(weights, np.float32)
    w_exp = weight_exponent(np.abs(weights).max() if weights.size else 0.0)
    cm, counters = kernel_counts(labels, preds, C, weights, w_exp)
    return np.ldexp(cm.astype(np.float64), -w_exp), counters, w_exp


def fixed_point_bound(labels, preds, C, weights):
    """per bin: 2^-23 |ref64| + k * max|w| * 2^-38, k the bin's element count, ref64 the float64 np.add.at sum -> (ref64, bound)"""
    labels, preds, weights = np.asarray(labels), np.asarray(preds), np.asarray(weights, np.float32)
    B = labels.shape[0]
    b = np.broadcast_to(np.arange(B)[:, None], labels.shape)
    ref = np.zeros((B, C, C), np.float64)
    np.add.at(ref, (b, labels, preds), weights.astype(np.float64))
    k = np.zeros((B, C, C), np.float64)
    np.add.at(k, (b, labels, preds), 1.0)
    return ref, 2.0 ** -23 * np.abs(ref) + k * float(np.abs(weights).max()) * 2.0 ** -38


def dynamic_range_case(n=1 << 18, C=5, seed=7):
    """Gaussian weights times 10^U(-6, 3): nine decades inside one matrix"""
    g = np.random.default_rng(seed)
    labels = g.integers(0, C, (1, n)).astype(np.int32)
    preds = g.integers(0, C, (1, n)).astype(np.int32)
    w = (g.standard_normal((1, n)) * 10.0 ** g.uniform(-6, 3, (1, n))).astype(np.float32)
    return labels, preds, w


# ---- launcher arithmetic (csrc/confusion.hip) ---------------------------------------------------------------------------------------------------
LDS_BYTES = 160 * 1024 - 64
LDS_MAX_BANDS = 4      # CM_LDS_MAX_BANDS: the LDS route up to this many bands, direct global atomics beyond
CUS = 256


def grid_cap(C, wmode):
    """workgroups per launch: what the CUs hold at once with this route's LDS, at most four per CU"""
    nbands, rows, kind = route(C, wmode)
    lds = 64 + (rows * C * (8 if wmode == W_F32 else 4) if kind == "lds" else 0)
    return CUS * min(4, (LDS_BYTES + 64) // lds)


def grid(batch, n, C=21, wmode=W_NONE):
    """(gx, gy, slices, trips): workgroups per image, images at a time, slices per image, trips of a workgroup's slice loop"""
    cap = grid_cap(C, wmode)
    slices = -(-n // SLICE)
    gy = min(batch, cap)
    gx = max(1, min(slices, cap // gy))
    return gx, gy, slices, -(-slices // gx)


def route(C, wmode):
    """(nbands, band_rows, "lds" | "global")"""
    bin_bytes = 8 if wmode == W_F32 else 4
    nbands, rows = 1, C
    while nbands <= 4 and rows * C * bin_bytes > LDS_BYTES:
        nbands += 1
        rows = -(-C // nbands)
    return (nbands, rows, "lds") if nbands <= LDS_MAX_BANDS else (1, C, "global")
