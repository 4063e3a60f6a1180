"""metrics/sod/fmeasurev2.py of the reference: TFBaseHandler (:22-298) and its ten handlers -- TFIOUHandler, TFSpecificityHandler (= TFTNRHandler),
TFDICEHandler, TFOverallAccuracyHandler, TFKappaHandler, TFPrecisionHandler, TFRecallHandler (= TFTPRHandler = TFSensitivityHandler), TFFPRHandler,
TFBERHandler, TFFmeasureHandler -- and the TFFmeasureV2 evaluator (:758-829), with their names, keyword arguments and defaults.

The scores come from csrc/sod_fmv2.hip (kernels.sod_fmv2): one streaming pass over pred and gt (a second one for an fp32 prediction when some
handler records the adaptive mode), a per-image finalize that evaluates every handler on the exact TP / FP / TN / FN, and a launch that adds to
the running state.  TFFmeasureV2 owns that state: one device buffer [n_handlers, 264] fp64 (0..255 the dynamic curve, 256 adaptive, 257 binary per
sample, 258..261 the binary tp, fp, tn, fn totals) and one int64 count -- every count of the reference equals the number of images.  One
`update_state` of the evaluator is ONE kernel call for all of its handlers and reads nothing back; `result()` sums the replicas' state through
dist.all_reduce_sum.  ISEG_SODFMV2_FUSED=0 (read at every call) selects the composed route of `composed_record` (bincount, cumsum, masked
counts) instead: the A/B partner, not a fallback.

`update_state(pred, gt, normalize=True)` takes one image [H,W], as the reference, or a batch [B,H,W] whose images are scored one by one.  With
normalize=True (the reference's default here) pred and gt are uint8 grey-level images (mapminmax of pred per image, gt > 128); with
normalize=False pred is float32 in [0,1] and gt bool / uint8 (non-zero = foreground).

A handler used alone owns a private evaluator of one.  A handler that belongs to an evaluator of several is updated and reset through the
evaluator; its own `update_state` / `reset_state` raise, because they would count or drop the images for every member.  Handlers join an
evaluator before its first update (or after a reset): the count is shared.  A handler that joins starts from zero.

Deviations from the reference:
  * counts and formulas are exact-integer / fp64 where the reference is fp32 (its TYPE): they differ only once a count passes 2^24, or where an
    fp32 rounding decides a safe_divide zero test (here the test is made on the integer denominator; Kappa's 1 - p_e == 0 is
    (tp+fp)(tp+fn) + (tn+fn)(tn+tp) == total^2 in integers).  The F-measure's beta is a double, not the fp32 constant of :739.
  * the histogram bin int(p * 255.0f) and the adaptive threshold keep their fp32 roundings (the mean behind the threshold is formed in fp64).
  * Kappa keeps the reference's own formula, (tn + fn) * (tn + tp) as its second product (:519).
"""
import os

import torch

from ... import nn
from . import sod_metric_utils as U
from .sod_metric_utils import safe_divide

KINDS = ("iou", "specificity", "dice", "overall_accuracy", "kappa", "precision", "recall", "fpr", "ber", "fmeasure")
IOU, SPECIFICITY, DICE, OA, KAPPA, PRECISION, RECALL, FPR, BER, FMEASURE = range(10)
DYNAMIC, ADAPTIVE, BINARY = 1, 2, 4
HANDLER_DOUBLES, MAX_HANDLERS = 264, 32
D_ADAPTIVE, D_BINARY, D_BINARY_COUNTS = 256, 257, 258


def _fused():
    return os.environ.get("ISEG_SODFMV2_FUSED", "1") != "0"


# ---------------------------------------------------------------------------------------------------------
# compute_metric (:336-749): on int64 tensors (the composed route) and on Python integers (the dataset-based binary result)
# ---------------------------------------------------------------------------------------------------------
def _sdiv(num, den):
    """safe_divide with the zero test on the integer denominator; num float64, den int64"""
    zero = den == 0
    return torch.where(zero, torch.zeros_like(num), num / torch.where(zero, torch.ones_like(den), den).to(torch.float64))


def metric_on_counts(kind, beta, tp, fp, tn, fn):
    """compute_metric of handler `kind` on int64 tensors of one shape, fp64 result; exact for totals below 2^31 (any single image)"""
    f = lambda v: v.to(torch.float64)      # noqa: E731
    if kind == IOU:
        return _sdiv(f(tp), tp + fp + fn)
    if kind == SPECIFICITY:
        return _sdiv(f(tn), tn + fp)
    if kind == DICE:
        return _sdiv(2.0 * f(tp), tp + fn + tp + fp)
    if kind == OA:
        return _sdiv(f(tp + tn), tp + fp + tn + fn)
    if kind == KAPPA:
        total = tp + fp + tn + fn
        agree, total2 = (tp + fp) * (tp + fn) + (tn + fn) * (tn + tp), total * total      # the reference's formula (:519)
        oa, hpy = _sdiv(f(tp + tn), total), _sdiv(f(agree), total2)
        d = 1.0 - hpy
        zero = ((total2 != 0) & (agree == total2)) | (d == 0.0)
        return torch.where(zero, torch.zeros_like(d), (oa - hpy) / torch.where(zero, torch.ones_like(d), d))
    if kind == PRECISION:
        return _sdiv(f(tp), tp + fp)
    if kind == RECALL:
        return _sdiv(f(tp), tp + fn)
    if kind == FPR:
        return _sdiv(f(fp), tn + fp)
    if kind == BER:
        return 1.0 - 0.5 * (_sdiv(f(tp), tp + fn) + _sdiv(f(tn), tn + fp))
    if kind == FMEASURE:
        pre, rec = _sdiv(f(tp), tp + fp), _sdiv(f(tp), tp + fn)
        den = beta * pre + rec
        zero = den == 0.0
        return torch.where(zero, torch.zeros_like(den), (beta + 1.0) * pre * rec / torch.where(zero, torch.ones_like(den), den))
    raise ValueError(f"unknown handler kind {kind}")


def metric_on_totals(kind, beta, tp, fp, tn, fn):
    """the same on Python integers of any size (counts summed over a dataset), a float"""
    d = lambda a, b: 0.0 if b == 0 else a / b      # noqa: E731
    if kind == IOU:
        return d(tp, tp + fp + fn)
    if kind == SPECIFICITY:
        return d(tn, tn + fp)
    if kind == DICE:
        return d(2 * tp, tp + fn + tp + fp)
    if kind == OA:
        return d(tp + tn, tp + fp + tn + fn)
    if kind == KAPPA:
        total = tp + fp + tn + fn
        agree = (tp + fp) * (tp + fn) + (tn + fn) * (tn + tp)
        oa, hpy = d(tp + tn, total), d(agree, total * total)
        return 0.0 if (total and agree == total * total) or 1.0 - hpy == 0.0 else (oa - hpy) / (1.0 - hpy)
    if kind == PRECISION:
        return d(tp, tp + fp)
    if kind == RECALL:
        return d(tp, tp + fn)
    if kind == FPR:
        return d(fp, tn + fp)
    if kind == BER:
        return 1.0 - 0.5 * (d(tp, tp + fn) + d(tn, tn + fp))
    if kind == FMEASURE:
        pre, rec = d(tp, tp + fp), d(tp, tp + fn)
        den = beta * pre + rec
        return 0.0 if den == 0.0 else (beta + 1.0) * pre * rec / den
    raise ValueError(f"unknown handler kind {kind}")


# ---------------------------------------------------------------------------------------------------------
# the composed route
# ---------------------------------------------------------------------------------------------------------
def composed_record(pred, gt, handlers):
    """the per-image record [n, 264] fp64 (layout: include/iseg_hip.h) of one image, pred fp32 [H,W] in [0,1] and gt bool [H,W]; handlers a
    sequence of (kind, modes, beta).  Tensor ops only, nothing is read back."""
    dev = pred.device
    out = torch.zeros(len(handlers), HANDLER_DOUBLES, dtype=torch.float64, device=dev)
    FG = gt.sum()
    BG = gt.numel() - FG

    def stats(binary):
        tp = (binary & gt).sum()
        fp = binary.sum() - tp
        return tp, fp, BG - fp, FG - tp

    bins = (pred * 255.0).to(torch.int64).clamp(0, 255)
    tps = torch.cumsum(torch.flip(torch.bincount(bins[gt], minlength=256), [0]), 0)
    fps = torch.cumsum(torch.flip(torch.bincount(bins[~gt], minlength=256), [0]), 0)
    dyn = (tps, fps, BG - fps, FG - tps)
    adp = stats(pred >= U.get_adaptive_threshold(pred)) if any(m & ADAPTIVE for _, m, _ in handlers) else None
    bny = stats(pred > 0.5)
    for h, (kind, modes, beta) in enumerate(handlers):
        if modes & DYNAMIC:
            out[h, :256] = metric_on_counts(kind, beta, *dyn)
        if modes & ADAPTIVE:
            out[h, D_ADAPTIVE] = metric_on_counts(kind, beta, *adp)
        if modes & BINARY:
            out[h, D_BINARY] = metric_on_counts(kind, beta, *bny)
            out[h, D_BINARY_COUNTS:D_BINARY_COUNTS + 4] = torch.stack(bny).to(torch.float64)
    return out


# ---------------------------------------------------------------------------------------------------------
# the evaluator and the handlers
# ---------------------------------------------------------------------------------------------------------
class TFFmeasureV2:
    """Running state of its handlers on one device buffer, and the one place that launches the kernel."""

    def __init__(self, metric_handlers=None, name="fmeasure_v2", **kwargs):
        self.name = name
        self._kwargs = dict(kwargs)
        self._metric_handlers = metric_handlers if metric_handlers else {}
        self.count = torch.zeros(1, dtype=torch.int64, device=nn.device())
        self._updated = False
        self._layout()

    def _layout(self):
        hs = list(self._metric_handlers.values())
        if len(hs) > MAX_HANDLERS:
            raise ValueError(f"TFFmeasureV2 '{self.name}': {len(hs)} handlers, one call scores at most {MAX_HANDLERS}")
        for h in hs:
            h._evaluator = self
        self.state = torch.zeros(len(hs), HANDLER_DOUBLES, dtype=torch.float64, device=self.count.device)

    def add_handler(self, handler_name, metric_handler):
        if self._updated:
            raise RuntimeError(f"TFFmeasureV2 '{self.name}' has counted images already and its handlers share one count: add handlers before the "
                               "first update_state(), or after reset_state()")
        self._metric_handlers[handler_name] = metric_handler
        self._layout()

    def _table(self):
        return [(h.KIND, h._modes(), h._beta()) for h in self._metric_handlers.values()]

    def update_state(self, pred, gt, normalize=True):
        if not self._metric_handlers:
            raise ValueError("Please add your metric handler before using `update_state()`.")
        if pred.dim() == 2:
            pred, gt = pred[None], gt[None]
        if pred.dim() != 3 or tuple(pred.shape) != tuple(gt.shape):
            raise ValueError("Shape mismatch between prediction and ground truth")
        if not normalize and pred.dtype != torch.float32:
            pred = pred.to(torch.float32)
        if gt.dtype not in (torch.bool, torch.uint8):
            gt = gt != 0
        if self.state.device != pred.device:
            self.state, self.count = self.state.to(pred.device), self.count.to(pred.device)
        self._updated = True
        table = self._table()
        if _fused():
            from ... import kernels as K

            K.sod_fmv2(pred.contiguous(), gt.contiguous(), table, normalize=normalize, state=self.state, count=self.count)
        else:
            p, g = U.validate_and_normalize_input(pred, gt if normalize else gt != 0, normalize)
            for b in range(p.shape[0]):
                self.state += composed_record(p[b], g[b], table)
            self.count += p.shape[0]

    def reduced(self):
        """(state, count) summed over the replicas, on the host"""
        from ... import dist

        s, c = self.state.clone(), self.count.clone()
        dist.all_reduce_sum(s)
        dist.all_reduce_sum(c)
        return s.cpu(), c.cpu()

    def result(self):
        s, c = self.reduced()
        return {name: h._result(s[i], c) for i, (name, h) in enumerate(self._metric_handlers.items())}

    def reset_state(self):
        self.state.zero_()
        self.count.zero_()
        self._updated = False

    reset_states = reset_state

    def get_config(self):
        return {"name": self.name, "dtype": "float32", **self._kwargs}


class TFBaseHandler:
    KIND = None

    def __init__(self, with_dynamic, with_adaptive, *, with_binary=False, sample_based=True, name="base_handler", **kwargs):
        self.name = name
        self._kwargs = dict(kwargs)
        self.with_dynamic = bool(with_dynamic)
        self.with_adaptive = bool(with_adaptive)
        self.with_binary = bool(with_binary)
        self.sample_based = bool(sample_based)
        self._evaluator = None      # an evaluator of its own, made at the first use, unless it joins a shared one first

    def _modes(self):
        return (DYNAMIC if self.with_dynamic else 0) | (ADAPTIVE if self.with_adaptive else 0) | (BINARY if self.with_binary else 0)

    def _beta(self):
        return 0.0

    def _own(self):
        if self.KIND is None:
            raise NotImplementedError("TFBaseHandler is abstract: use one of the ten handlers")
        if self._evaluator is None:
            TFFmeasureV2({self.name: self}, name=self.name)
        return self._evaluator

    def _alone(self, what):
        ev = self._own()
        if len(ev._metric_handlers) > 1:
            raise RuntimeError(f"handler '{self.name}' belongs to a TFFmeasureV2 of {len(ev._metric_handlers)} handlers that share one state: call "
                               f"the evaluator's {what} once, it covers every member")
        return ev

    def compute_metric(self, tp, fp, tn, fn):
        """the handler's formula on counts (numbers or tensors of one shape), fp64"""
        if self.KIND is None:
            raise NotImplementedError("TFBaseHandler is abstract: use one of the ten handlers")
        tp, fp, tn, fn = (torch.as_tensor(v).to(torch.float64).round().to(torch.int64) for v in (tp, fp, tn, fn))
        return metric_on_counts(self.KIND, self._beta(), tp, fp, tn, fn)

    def update_state(self, pred, gt, normalize=True):
        self._alone("update_state(pred, gt)").update_state(pred, gt, normalize)

    def reset_state(self):
        self._alone("reset_state()").reset_state()

    reset_states = reset_state

    def _result(self, row, count):
        """row [264] fp64 and count [1] int64, summed over the replicas, on the host"""
        c = count.to(torch.float64)
        results = {}
        if self.with_dynamic:
            results["dynamic"] = safe_divide(row[:256], c.expand(256))
        if self.with_adaptive:
            results["adaptive"] = safe_divide(row[D_ADAPTIVE:D_ADAPTIVE + 1], c)[0]
        if self.with_binary:
            if self.sample_based:
                results["binary"] = safe_divide(row[D_BINARY:D_BINARY + 1], c)[0]
            else:
                tp, fp, tn, fn = (int(v) for v in row[D_BINARY_COUNTS:D_BINARY_COUNTS + 4].tolist())
                results["binary"] = torch.tensor(metric_on_totals(self.KIND, self._beta(), tp, fp, tn, fn), dtype=torch.float32)
        return results

    def result(self):
        ev = self._own()
        s, c = ev.reduced()
        return self._result(s[list(ev._metric_handlers.values()).index(self)], c)

    def get_config(self):
        return {"name": self.name, "dtype": "float32", **self._kwargs, "with_dynamic": self.with_dynamic, "with_adaptive": self.with_adaptive,
                "with_binary": self.with_binary, "sample_based": self.sample_based}


def _handler(kind, default_name, doc):
    class Handler(TFBaseHandler):
        KIND = kind

        def __init__(self, with_dynamic, with_adaptive, *, with_binary=False, sample_based=True, name=default_name, **kwargs):
            super().__init__(with_dynamic, with_adaptive, with_binary=with_binary, sample_based=sample_based, name=name, **kwargs)

    Handler.__doc__ = doc
    return Handler


TFIOUHandler = _handler(IOU, "iou", "iou = tp / (tp + fp + fn)")
TFSpecificityHandler = _handler(SPECIFICITY, "specificity", "specificity = tn / (tn + fp)")
TFDICEHandler = _handler(DICE, "dice", "dice = 2 tp / (tp + fn + tp + fp)")
TFOverallAccuracyHandler = _handler(OA, "overall_accuracy", "oa = (tp + tn) / (tp + fp + tn + fn)")
TFKappaHandler = _handler(KAPPA, "kappa", "kappa = (oa - p_e) / (1 - p_e), p_e = [(tp + fp)(tp + fn) + (tn + fn)(tn + tp)] / total^2")
TFPrecisionHandler = _handler(PRECISION, "precision", "precision = tp / (tp + fp)")
TFRecallHandler = _handler(RECALL, "recall", "recall = tp / (tp + fn)")
TFFPRHandler = _handler(FPR, "fpr", "fpr = fp / (tn + fp)")
TFBERHandler = _handler(BER, "ber", "ber = 1 - (tp / (tp + fn) + tn / (tn + fp)) / 2")
for _cls, _name in ((TFIOUHandler, "TFIOUHandler"), (TFSpecificityHandler, "TFSpecificityHandler"), (TFDICEHandler, "TFDICEHandler"),
                    (TFOverallAccuracyHandler, "TFOverallAccuracyHandler"), (TFKappaHandler, "TFKappaHandler"),
                    (TFPrecisionHandler, "TFPrecisionHandler"), (TFRecallHandler, "TFRecallHandler"), (TFFPRHandler, "TFFPRHandler"),
                    (TFBERHandler, "TFBERHandler")):
    _cls.__name__ = _cls.__qualname__ = _name
TFTNRHandler = TFSpecificityHandler
TFTPRHandler = TFRecallHandler
TFSensitivityHandler = TFRecallHandler


class TFFmeasureHandler(TFBaseHandler):
    """fmeasure = (beta + 1) precision recall / (beta precision + recall); beta multiplies as the reference writes it (not squared)"""
    KIND = FMEASURE

    def __init__(self, with_dynamic, with_adaptive, *, with_binary=False, sample_based=True, beta=0.3, name="fmeasure", **kwargs):
        super().__init__(with_dynamic, with_adaptive, with_binary=with_binary, sample_based=sample_based, name=name, **kwargs)
        self.beta = float(beta)

    def _beta(self):
        return self.beta

    def get_config(self):
        return {**super().get_config(), "beta": self.beta}
