"""NumPy restatement of the reference's FmeasureV2 handlers (metrics/sod/fmeasurev2.py), written from its formulas.

Counts are exact integers; the scores are fp64 on them.  What the reference's fp32 decides discretely is kept in fp32 through
tests/sod_metrics_ref.py: the bin int(p * 255.0) is an np.float32 product (fmeasurev2.py:211), the adaptive threshold is min(2 mean, 1) rounded to
fp32 and compared in fp32 (sod_metric_utils.py:98-109), prepare_data's mapminmax runs in fp32 (sod_metric_utils.py:82-95), and binary is
p > 0.5 in fp32 (fmeasurev2.py:145).  safe_divide (sod_metric_utils.py:138-152) returns 0 where the denominator is 0; with exact counts that is a
test on the integer.  Kappa's last division tests 1 - p_e == 0, which with exact counts is (tp+fp)(tp+fn) + (tn+fn)(tn+tp) == total^2.
"""
import numpy as np

from tests import sod_metrics_ref as S

KINDS = ("iou", "specificity", "dice", "overall_accuracy", "kappa", "precision", "recall", "fpr", "ber", "fmeasure")


def safe_divide(num, den):
    """sod_metric_utils.py:138-152"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))


def compute_metric(kind, tp, fp, tn, fn, beta=0.3):
    """fmeasurev2.py:336-749 on integer counts (scalars or arrays), fp64"""
    tp, fp, tn, fn = (np.asarray(v, np.int64) for v in (tp, fp, tn, fn))
    if kind == "iou":                   # :340
        return safe_divide(tp, tp + fp + fn)
    if kind == "specificity":           # :382
        return safe_divide(tn, tn + fp)
    if kind == "dice":                  # :428
        return safe_divide(2.0 * tp, tp + fn + tp + fp)
    if kind == "overall_accuracy":      # :470
        return safe_divide(tp + tn, tp + fp + tn + fn)
    if kind == "kappa":                 # :514-523, the second product as the reference writes it
        total = tp + fp + tn + fn
        oa = safe_divide(tp + tn, total)
        agree = (tp + fp) * (tp + fn) + (tn + fn) * (tn + tp)
        hpy = safe_divide(agree, total * total)
        one = (agree == total * total) & (total != 0)      # 1 - hpy == 0 on the integers
        return np.where(one, 0.0, (oa - hpy) / np.where(one, 1.0, 1.0 - hpy))
    if kind == "precision":             # :565
        return safe_divide(tp, tp + fp)
    if kind == "recall":                # :607
        return safe_divide(tp, tp + fn)
    if kind == "fpr":                   # :654
        return safe_divide(fp, tn + fp)
    if kind == "ber":                   # :696-700
        return 1.0 - 0.5 * (safe_divide(tp, tp + fn) + safe_divide(tn, tn + fp))
    if kind == "fmeasure":              # :745-749
        precision, recall = safe_divide(tp, tp + fp), safe_divide(tp, tp + fn)
        return safe_divide((beta + 1.0) * precision * recall, beta * precision + recall)
    raise ValueError(kind)


def get_statistics(binary, gt):
    """fmeasurev2.py:156-177: (tp, fp, tn, fn)"""
    FG = int(np.count_nonzero(gt))
    BG = gt.size - FG
    TP = int(np.count_nonzero(binary[gt]))
    FP = int(np.count_nonzero(binary[~gt]))
    return TP, FP, BG - FP, FG - TP


def integers(pred, gt):
    """every integer of one image (pred fp32 [H,W] in [0,1], gt bool [H,W]): histograms, foreground count, adaptive and binary counts, threshold"""
    fg, bg = S.histograms(pred, gt)
    thr = S.adaptive_threshold(pred)
    ge = pred.astype(np.float32) >= thr
    hi = pred.astype(np.float32) > np.float32(0.5)
    return dict(hist_fg=fg, hist_bg=bg, nfg=int(np.count_nonzero(gt)), nge=int(ge.sum()), ngefg=int((ge & gt).sum()), n05=int(hi.sum()),
                n05fg=int((hi & gt).sum()), thr=thr)


def counts(pred, gt):
    """(dynamic, adaptive, binary), each (tp, fp, tn, fn); the dynamic ones are arrays [256], index i is threshold 255 - i (:229-237)"""
    w = integers(pred, gt)
    FG = w["nfg"]
    BG = gt.size - FG
    TPs, FPs = np.cumsum(w["hist_fg"][::-1]), np.cumsum(w["hist_bg"][::-1])
    dyn = (TPs, FPs, BG - FPs, FG - TPs)
    adp = get_statistics(pred.astype(np.float32) >= w["thr"], gt)
    bny = get_statistics(pred.astype(np.float32) > np.float32(0.5), gt)
    return dyn, adp, bny


def all_handlers(pred, gt, beta=0.3):
    """{"ints": integers(), "binary_counts": (tp, fp, tn, fn), kind: {"dynamic": [256], "adaptive": float, "binary": float}} for one image"""
    dyn, adp, bny = counts(pred, gt)
    out = {"ints": integers(pred, gt), "binary_counts": bny}
    for kind in KINDS:
        out[kind] = {"dynamic": compute_metric(kind, *dyn, beta=beta), "adaptive": float(compute_metric(kind, *adp, beta=beta)),
                     "binary": float(compute_metric(kind, *bny, beta=beta))}
    return out
