"""NumPy restatement of losses/ohem.py:11-39 of the reference (test-only), literal: descending sort, strict compares, the index taken as written.

    thresh given:  prob = max_c softmax(y_pred)_c * onehot_c  (0 on a zero row);  nnz = count_nonzero(prob);
                   k = min(min_kept * batch_size, nnz - 1) if nnz > 0;  min_threshold = sort(prob, DESCENDING)[k], or 0 if nnz == 0;
                   threshold = max(min_threshold, thresh);  out = loss where prob < threshold, else 0
    thresh None:   threshold = sort(loss, DESCENDING)[min_kept * batch_size]  (ValueError past the end);  out = loss where loss > threshold, else 0

select_values() is the selection alone on a given array, in that array's own precision (fp32 in: exact fp32 compares); ohem() computes the
probabilities in fp64 from logits and integer labels first.  The label-to-row rule is the one of the ignore-label cross-entropy
(losses/catecrossentropy_ignore_label.py:56-61): ignore_label == 0 shifts the labels down by one, a class outside [0, C) is the zero row."""
import numpy as np


def label_rows(labels, ignore_label, num_class):
    """(class per position, True where the one-hot row is not the zero row)"""
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    if ignore_label == 0:
        y = y - 1
    return y, (y >= 0) & (y < num_class)


def label_prob(logits, labels, ignore_label):
    """fp64 probability of the labelled class [P], exactly 0 on a zero row"""
    z = np.asarray(logits, np.float64)
    z = z.reshape(-1, z.shape[-1])
    y, in_range = label_rows(labels, ignore_label, z.shape[1])
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return np.where(in_range, p[np.arange(z.shape[0]), np.clip(y, 0, z.shape[1] - 1)], 0.0)


def select_values(values, loss, min_kept_total, thresh):
    """the selection alone.  thresh a number: values is prob; thresh None: values is the loss.  -> dict(threshold, nnz, k, keep, out)"""
    v = np.asarray(values).reshape(-1)
    loss = np.asarray(loss).reshape(-1)
    nnz = int(np.count_nonzero(v))
    descending = np.sort(v)[::-1]
    if thresh is not None:
        if nnz > 0:
            k = min(int(min_kept_total), nnz - 1)
            min_threshold = descending[k]
        else:
            k, min_threshold = None, v.dtype.type(0)
        threshold = np.maximum(min_threshold, v.dtype.type(thresh))
        keep = v < threshold
    else:
        k = int(min_kept_total)
        if not 0 <= k < v.size:
            raise ValueError(f"index {k} of {v.size} sorted losses")
        threshold = descending[k]
        keep = v > threshold
    return dict(threshold=threshold, nnz=nnz, k=k, keep=keep, out=np.where(keep, loss, loss.dtype.type(0)))


def ohem(logits, labels, loss, ignore_label, batch_size, thresh, min_kept):
    """ohem_selector with fp64 probabilities; with thresh None the selection runs on `loss` as given"""
    values = np.asarray(loss).reshape(-1) if thresh is None else label_prob(logits, labels, ignore_label)
    res = select_values(values, loss, int(min_kept) * int(batch_size), thresh)
    res["values"] = values
    return res
