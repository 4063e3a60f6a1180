"""metrics/sod/sod_metrics.py of the reference: TFMAEMetric (:114-190), TFSmeasureMetric (:193-438), TFEmeasureMetric (:441-743),
TFFmeasureMetric (:746-938) and TFWeightedFmeasureMetric (:941-1076), with their class names, constructor arguments and defaults.

The scores come from csrc/sod_metrics.hip (kernels.sod_metrics): two streaming passes over pred and gt, the weighted F-measure's distance
transform and Gaussian, one per-image finalize, and a launch that adds to the running state.  The state lives on the device (fp64 sums, an int64
count), `update_state` reads nothing back, and `result()` sums the replicas' state through dist.all_reduce_sum, as MeanIOU does.
ISEG_SODMETRICS_FUSED=0 (read at every call) selects the composed route of sod_metric_utils.composed_record instead: the A/B partner.

`update_state(pred, gt, normalize=False)` takes one image [H,W], as the reference, or a batch [B,H,W] whose images are scored one by one.
pred is float32 in [0,1] and gt bool / uint8 (non-zero = foreground); with normalize=True pred and gt are uint8 grey-level images
(mapminmax of pred per image, gt > 128).

`result()` is what the reference returns today: sum / count through safe_divide, and for E and F the mean of the curve.  The adaptive scores
and the curves, which the reference computes and drops, are `adaptive_result()`, `curve_result()`, `precision_curve()`, `recall_curve()`.

Metrics updated together on the same (pred, gt) go into a SodMetricSet, which runs the shared passes ONCE for all of them.  Members of a
set of several metrics are updated through the set; `update_state` on one of them raises, because it would count the image for every member.

Deviations from the reference, all where its fp32 formula is not finite or not determined:
  * a centroid quadrant of the S-measure without pixels (the centroid on the last row or column) contributes 0; the reference multiplies a NaN by
    its zero weight.  A quadrant of ONE pixel has variances 0 (the reference divides 0 by 0), so _ssim's ladder gives 1 for it.
  * every sum is fp64 (the reference accumulates fp32); the histogram bin and the adaptive threshold keep their fp32 roundings.
  * equidistant foreground pixels in the weighted F-measure: the smallest row-major index is the nearest one (SciPy does not specify its choice).
"""
import os

import torch

from ... import nn
from . import sod_metric_utils as U
from .sod_metric_utils import safe_divide


def _fused():
    return os.environ.get("ISEG_SODMETRICS_FUSED", "1") != "0"


class SodMetricSet:
    """Running state of the five metrics on one device buffer, and the one place that launches the kernels.  Metrics passed in share this
    state: update them through the set (`set.update_state(pred, gt)`), one call of the shared passes for all of them."""

    def __init__(self, *metrics):
        self.metrics = list(metrics[0]) if len(metrics) == 1 and isinstance(metrics[0], (list, tuple)) else list(metrics)
        self.state = torch.zeros(U.STATE_DOUBLES, dtype=torch.float64, device=nn.device())
        self.count = torch.zeros(1, dtype=torch.int64, device=nn.device())
        for m in self.metrics:
            m._set = self
        self._params()

    def _params(self):
        p = dict(alpha=0.5, beta_fm=0.3, beta_wfm=1.0)
        for m in self.metrics:
            p.update(m._kernel_params())
        self.params = p
        self.wfm = any(m._needs_wfm for m in self.metrics)

    def update_state(self, pred, gt, normalize=False):
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
        if _fused():
            from ... import kernels as K

            K.sod_metrics(pred.contiguous(), gt.contiguous(), normalize=normalize, wfm=self.wfm, state=self.state, count=self.count, **self.params)
        else:
            p, g = U.validate_and_normalize_input(pred, gt if normalize else gt != 0, normalize)
            for b in range(p.shape[0]):
                self.state += U.composed_record(p[b], g[b], wfm=self.wfm, **self.params)
            self.count += p.shape[0]

    def reset_state(self):
        self.state.zero_()
        self.count.zero_()

    def reduced(self):
        """(state, count) summed over the replicas, on the host"""
        from ... import dist

        s, c = self.state.clone(), self.count.clone()
        dist.all_reduce_sum(s)
        dist.all_reduce_sum(c)
        return s.cpu(), c.cpu()


class _SodMetric:
    _needs_wfm = False

    def __init__(self, name, **kwargs):
        self.name = name
        self._kwargs = dict(kwargs)
        self._set = None      # a set of its own, made at the first use, unless it joins a shared one first

    def _own(self):
        if self._set is None:
            SodMetricSet(self)
        return self._set

    def _kernel_params(self):
        return {}

    def update_state(self, pred, gt, normalize=False):
        st = self._own()
        if len(st.metrics) > 1:
            raise RuntimeError(f"metric '{self.name}' belongs to a SodMetricSet of {len(st.metrics)} metrics that share one state: call the set's "
                               "update_state(pred, gt) once, it updates every member")
        st._params()
        st.update_state(pred, gt, normalize)

    def reset_state(self):
        self._own().reset_state()

    reset_states = reset_state

    def _mean(self, lo, n=1):
        s, c = self._own().reduced()
        v = safe_divide(s[lo:lo + n], c.to(torch.float64).expand(n))
        return v[0] if n == 1 else v

    def get_config(self):
        return {"name": self.name, "dtype": "float32", **self._kwargs}


class TFMAEMetric(_SodMetric):
    def __init__(self, name="mae", **kwargs):
        super().__init__(name, **kwargs)

    def result(self):
        return self._mean(U.S_MAE)


class TFSmeasureMetric(_SodMetric):
    def __init__(self, alpha=0.5, name="sm", **kwargs):
        self.alpha = float(alpha)
        super().__init__(name, **kwargs)

    def _kernel_params(self):
        return {"alpha": self.alpha}

    def result(self):
        return self._mean(U.S_SM)

    def get_config(self):
        return {**super().get_config(), "alpha": self.alpha}


class TFEmeasureMetric(_SodMetric):
    def __init__(self, name="em", **kwargs):
        super().__init__(name, **kwargs)

    def curve_result(self):
        """the 256-point E-measure curve; index i is threshold 255 - i"""
        return self._mean(U.S_EM, 256)

    def adaptive_result(self):
        return self._mean(U.S_EM_ADP)

    def result(self):
        return self.curve_result().mean()


class TFFmeasureMetric(_SodMetric):
    def __init__(self, beta=0.3, name="fm", **kwargs):
        self.beta = float(beta)
        super().__init__(name, **kwargs)

    def _kernel_params(self):
        return {"beta_fm": self.beta}

    def curve_result(self):
        """the 257-point F-measure curve; index i is threshold 256 - i"""
        return self._mean(U.S_FM, 257)

    def precision_curve(self):
        return self._mean(U.S_PREC, 257)

    def recall_curve(self):
        return self._mean(U.S_REC, 257)

    def adaptive_result(self):
        return self._mean(U.S_FM_ADP)

    def result(self):
        return self.curve_result().mean()

    def get_config(self):
        return {**super().get_config(), "beta": self.beta}


class TFWeightedFmeasureMetric(_SodMetric):
    _needs_wfm = True

    def __init__(self, beta=1.0, name="wfm", **kwargs):
        self.beta = float(beta)
        super().__init__(name, **kwargs)

    def _kernel_params(self):
        return {"beta_wfm": self.beta}

    def result(self):
        return self._mean(U.S_WFM)

    def get_config(self):
        return {**super().get_config(), "beta": self.beta}
