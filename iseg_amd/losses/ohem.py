"""losses/ohem.py of the reference (:11-46): online hard example mining on the per-position loss vector, restated literally.

ohem_selector(loss, y_true, y_pred, batch_size, thresh, min_kept) works on flattened positions: loss [P], y_pred [P, C] logits, y_true the
one-hot rows [P, C] (an all-zero row for a label outside [0, C)).

    thresh given:  prob = max_c softmax(y_pred)_c * y_true_c;  nnz = count_nonzero(prob);  k = min(min_kept * batch_size, nnz - 1);
                   threshold = max(sort(prob, DESCENDING)[k], thresh)  (max(0, thresh) when nnz == 0);  loss where prob < threshold, else 0
    thresh None:   threshold = sort(loss, DESCENDING)[min_kept * batch_size];  loss where loss > threshold, else 0

The sort is DESCENDING, so with the reference's defaults (min_kept = 100000 per image) k is nnz - 1, the threshold is
max(smallest non-zero probability, thresh), and every labelled pixel the model gives less than `thresh` is kept.  That is what the reference
computes and what this does; it is not "repaired" into the ascending-sort OHEM of the literature.

y_true may also be the flattened integer labels [P] (any value outside [0, C) is a zero row): that is what weighted_loss of
catecrossentropy_ignore_label_loss hands over, and what the kernels read.  One-hot rows are turned into such labels first.  The k-th
largest value comes from a radix select on the device (csrc/ohem.hip); nothing is read back, and under data parallelism every rank
selects over its own positions, as each replica does in the reference."""
import torch

from .. import functional as F


def _labels_of(y_true, y_pred):
    """flattened integer labels [P]; one-hot rows (the shape of y_pred) -> their class, -1 for an all-zero row"""
    if tuple(y_true.shape) != tuple(y_pred.shape):
        return y_true.reshape(-1)
    hot = y_true.reshape(-1, y_pred.shape[-1]) != 0
    cls = hot.to(torch.int32).argmax(dim=-1).to(torch.int32)
    return torch.where(hot.any(dim=-1), cls, torch.full_like(cls, -1))


def ohem_selector(loss, y_true, y_pred, batch_size=4, thresh=None, min_kept=100000):
    num_class = int(y_pred.shape[-1])
    labels = None if thresh is None else _labels_of(y_true, y_pred)
    # ignore_label -1: the labels are classes already, nothing is shifted
    return F.ohem_select_per_pixel(loss, y_pred, labels, num_class, -1, int(min_kept) * int(batch_size), thresh)


class _OhemFn:
    """what get_ohem_fn returns: wrapper_fn(y_true, y_pred, loss, batch_size) of the reference (:43-44), with thresh / min_kept readable so
    that catecrossentropy_ignore_label_loss can route the scalar loss through the fused selection"""

    def __init__(self, thresh, min_kept):
        self.thresh, self.min_kept = thresh, min_kept

    def __call__(self, y_true, y_pred, loss, batch_size):
        return ohem_selector(loss, y_true, y_pred, batch_size, self.thresh, self.min_kept)


def get_ohem_fn(thresh=None, min_kept=100000):
    return _OhemFn(thresh, min_kept)


def is_ohem_fn(fn):
    return isinstance(fn, _OhemFn)
