"""metrics/seg_metric_wrapper.py of the reference (:22-110): nearest-resize the label map to the logits size, argmax
(first maximal index), drop ignored labels, accumulate.  SegMetricWrapper does all of it in one launch on the logits; process_seg_metric_inputs
is the reference's free function for callers that want the maps."""
import torch

from .. import kernels as K


def process_seg_metric_inputs(y_true, y_pred, num_class=21, ignore_label=255, use_class_prob_as_pred=True, flatten_outputs=True,
                              set_ignore_label_to_zero=True):
    """:22-68 -- (y_true, y_pred, not_ignore_mask) for a label-map metric such as MeanIOU.update_state: the labels as int32, nearest-resized
    to the prediction's size when that is [N, H, W, C]; the prediction as the first maximal class (use_class_prob_as_pred) or as it is, int32;
    the mask float32 1 / 0 where the label is not / is ignore_label; labels shifted down by one when ignore_label == 0, and 0 under the mask
    when set_ignore_label_to_zero.  flatten_outputs: all three are [N*H*W]."""
    y_true = torch.as_tensor(y_true).to(torch.int32)
    if y_pred.dim() == 4:
        if y_true.dim() == 3:
            y_true = y_true.unsqueeze(-1)
        if tuple(y_true.shape[1:3]) != tuple(y_pred.shape[1:3]):
            y_true = K.resize_nearest_i32(y_true.contiguous(), y_pred.shape[1], y_pred.shape[2])
    if use_class_prob_as_pred:
        z = y_pred.reshape(-1, y_pred.shape[-1] if not flatten_outputs else num_class)
        if z.dtype != torch.float32:
            z = K.cast(z.contiguous(), torch.float32)
        pred = K.argmax_confusion(z.contiguous(), None, ignore_label, cm=None, want_pred=True)
        y_pred = pred if flatten_outputs else pred.reshape(y_pred.shape[:-1])
    else:
        y_pred = (y_pred.reshape(-1) if flatten_outputs else y_pred).to(torch.int32)
    if flatten_outputs:
        y_true = y_true.reshape(-1)
    not_ignore_mask = y_true != ignore_label
    if ignore_label == 0:
        y_true = y_true - 1
    if set_ignore_label_to_zero:
        y_true = torch.where(not_ignore_mask, y_true, torch.zeros_like(y_true))
    return y_true, y_pred, not_ignore_mask.to(torch.float32)


class SegMetricWrapper:
    def __init__(self, metric, num_class=21, ignore_label=255, name=None):
        self.name = name
        self.metric = metric
        self.num_class = num_class
        self.ignore_label = ignore_label
        self._pre_compute_fn_list = []

    def add_pre_compute_fn(self, fn):
        if fn is None:
            return
        self._pre_compute_fn_list.append(fn)

    def update_state(self, y_true, y_pred, sample_weight=None):
        for fn in self._pre_compute_fn_list:
            y_true, y_pred = fn(y_true, y_pred)
        y_true = y_true.to(torch.int32)
        if y_pred.dim() == 4:
            if y_true.dim() == 3:
                y_true = y_true.unsqueeze(-1)
            if tuple(y_true.shape[1:3]) != tuple(y_pred.shape[1:3]):
                y_true = K.resize_nearest_i32(y_true.contiguous(), y_pred.shape[1], y_pred.shape[2])
        z = y_pred.reshape(-1, self.num_class)
        if z.dtype != torch.float32:
            z = K.cast(z.contiguous(), torch.float32)
        y = y_true.reshape(-1).contiguous()
        ignore = self.ignore_label
        if ignore == 0:
            # reference: mask = y != 0, then y -= 1 (process_seg_metric_inputs :56-59)
            y = y - 1
            ignore = -1
        self.metric.update_from_logits(z.contiguous(), y, ignore)

    def result(self):
        return self.metric.result()

    def reset_states(self):
        self.metric.reset_states()
