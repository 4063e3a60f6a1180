"""metrics/mean_iou.py of the reference (:16-153): confusion matrices of label maps, running confusion matrix -> per-class IoU -> mean
over the classes whose denominator is non-zero.  Counts are kept as exact uint64 on the device (the reference accumulates fp32)."""
import torch

from .. import nn
from .confusion_matrix import batch_confusion_matrix, confusion_matrix, raise_for_counters


def get_class_confusion_matrix(y_true, y_pred, num_class=21, sample_weight=None, dtype=torch.float32):
    """:16-34 -- every input flattened, one [num_class, num_class] matrix of `dtype`.  Float weights are summed in fixed point (see
    metrics/confusion_matrix.py); reads the kernel's counters back."""
    y_true, y_pred = torch.as_tensor(y_true).reshape(-1), torch.as_tensor(y_pred).reshape(-1)
    if sample_weight is not None:
        sample_weight = torch.as_tensor(sample_weight).reshape(-1)
    return confusion_matrix(y_true, y_pred, num_class, weights=sample_weight, dtype=dtype)


def get_batch_class_confusion_matrix(y_true, y_pred, num_class=21, sample_weight=None, dtype=torch.float32):
    """:38-55 -- every sample flattened, [B, num_class, num_class] of `dtype`"""
    y_true, y_pred = torch.as_tensor(y_true), torch.as_tensor(y_pred)
    B = y_true.shape[0]
    if sample_weight is not None:
        sample_weight = torch.as_tensor(sample_weight).reshape(B, -1)
    return batch_confusion_matrix(y_true.reshape(B, -1), y_pred.reshape(B, -1), num_class, weights=sample_weight, dtype=dtype)


def get_per_class_miou(cm, dtype=None, row_axis=-2, col_axis=-1):
    """:59-77 -- cm [..., C, C] (leading batch dimensions allowed) -> (iou [..., C], num_valid_entries [...]).  dtype None: the matrix is taken
    to float64 first and the result is float64; a dtype: the sums are taken in the matrix's own dtype and then cast, as the reference does.
    The diagonal is that of the last two axes whatever row_axis / col_axis say (tf.linalg.diag_part)."""
    if dtype is None:
        dtype = torch.float64
        cm = cm.to(dtype)
    sum_over_row = cm.sum(row_axis).to(dtype)
    sum_over_col = cm.sum(col_axis).to(dtype)
    tp = torch.diagonal(cm, dim1=-2, dim2=-1).to(dtype)
    denom = sum_over_row + sum_over_col - tp
    num_valid = (denom != 0).to(dtype).sum(-1)
    iou = torch.where(denom != 0, tp / torch.where(denom != 0, denom, torch.ones_like(denom)), torch.zeros_like(denom))
    return iou, num_valid


def per_class_miou_to_mean_miou(iou, num_valid_entries):
    s = iou.sum(-1)
    return torch.where(num_valid_entries != 0, s / torch.where(num_valid_entries != 0, num_valid_entries, torch.ones_like(s)),
                       torch.zeros_like(s))


class MeanIOU:
    def __init__(self, num_classes, name=None, dtype=None):
        self.name = name
        self.num_classes = num_classes
        self.total_cm = torch.zeros(num_classes * num_classes, dtype=torch.int64, device=nn.device())

    def update_from_logits(self, logits2d, labels1d, ignore_label):
        from .. import kernels as K

        K.argmax_confusion(logits2d, labels1d, ignore_label, cm=self.total_cm)

    def update_state(self, y_true, y_pred, sample_weight=None):
        """:112-130 -- adds the confusion matrix of two label maps (any shape, flattened) to total_cm, on the device, exactly.  total_cm holds
        integer counts, so the weights are none, bool / integer, or integer-valued floats (the 0 / 1 not-ignore mask of
        metrics/seg_metric_wrapper.py:102); a fractional weight raises ValueError and leaves total_cm as it was: use
        get_class_confusion_matrix for those.  Negative or out-of-bound labels / predictions raise the reference's messages (the valid
        elements of such a call have been counted).  Reads the kernel's counters back: a host synchronisation."""
        from .. import kernels as K

        y_true, y_pred = torch.as_tensor(y_true), torch.as_tensor(y_pred)
        if y_true.numel() != y_pred.numel():
            raise ValueError(f"MeanIOU.update_state: y_true and y_pred differ in size: {tuple(y_true.shape)} and {tuple(y_pred.shape)}")
        if sample_weight is not None:
            sample_weight = torch.as_tensor(sample_weight)
            if sample_weight.numel() != y_pred.numel():
                raise ValueError(f"MeanIOU.update_state: sample_weight has {sample_weight.numel()} elements, y_pred {y_pred.numel()}")
        K._require_cuda(y_true, y_pred, sample_weight)
        if y_pred.numel() == 0:
            return self.total_cm
        y = y_true.to(torch.int32).reshape(1, -1).contiguous()
        p = y_pred.to(torch.int32).reshape(1, -1).contiguous()
        w = None
        if sample_weight is not None:
            w = sample_weight.reshape(1, -1)
            w = w.contiguous() if w.dtype in (torch.bool, torch.uint8) else w.to(torch.float32).contiguous()
        _, counters = K.confusion_batched(y, p, self.num_classes, weights=w, w_exp=0, cm=self.total_cm, accumulate=True)
        c = [int(v) for v in counters.tolist()]
        if c[5]:
            # llrint is odd under round-to-nearest-even: the negated weights take out exactly what was added
            K.confusion_batched(y, p, self.num_classes, weights=-w, w_exp=0, cm=self.total_cm, accumulate=True)
            raise ValueError(f"MeanIOU.update_state: {c[5]} weights are not integers; total_cm keeps exact counts -- use "
                             "get_class_confusion_matrix for fractional weights")
        raise_for_counters(counters, "MeanIOU.update_state")
        return self.total_cm

    def per_class_result(self):
        cm = self.total_cm.clone()
        from .. import dist

        dist.all_reduce_sum(cm)     # C3 of SURVEY 2.2: replicas' confusion matrices are summed when the result is read
        return get_per_class_miou(cm.reshape(self.num_classes, self.num_classes).cpu())

    def result(self):
        iou, n = self.per_class_result()
        return per_class_miou_to_mean_miou(iou, n)

    def local_result(self):
        """mean IoU of THIS replica's counts only -- no collective, safe to call from one rank (progress lines)"""
        iou, n = get_per_class_miou(self.total_cm.reshape(self.num_classes, self.num_classes).cpu())
        return per_class_miou_to_mean_miou(iou, n)

    def reset_states(self):
        self.total_cm.zero_()
