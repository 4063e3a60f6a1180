"""metrics/confusion_matrix.py of the reference (:13-231): remove_squeezable_dimensions, confusion_matrix, batch_confusion_matrix, on the
integer-only kernel of csrc/confusion.hip.  Names, argument order and defaults are the reference's (its `name` argument has no meaning here).

How the weights are counted
  * none: every element adds 1;  bool / uint8: every element adds its byte;  both are exact.
  * every other integer dtype and every float dtype: cast to float32, then accumulated in FIXED POINT: an element adds
    llrint(w * 2^w_exp) to a 64-bit integer bin, with w_exp chosen from max |w| so that the largest weight lands in [2^37, 2^38).  A bin's
    value differs from the real sum of its k weights by at most k * max|w| * 2^-38, and it does not depend on the order of the elements: two
    calls, or any permutation of the elements, give the same bits.  The int64 sums come back as ldexp(cm.double(), -w_exp).to(dtype); an
    integer `dtype` with fractional weights therefore truncates toward zero AFTER the sum (the reference casts every weight to `dtype` first).
    At most 2^24 elements per image with such weights.
  * a weight that is NaN or infinite raises ValueError -- a departure from the reference, which would carry the NaN into the matrix.

Both functions read back from the device before they return: max |w| (four bytes, before the launch, to choose w_exp), and the kernel's
rejection counters (to raise the reference's assertion messages as ValueError).  They are host synchronisations by design; a caller that
wants none uses iseg_amd.kernels.confusion_batched.  There is no CPU path: tensors live on the device.
"""
import torch

from .. import kernels as K

_MESSAGES = ("`labels` contains negative values", "`predictions` contains negative values", "`labels` out of bound", "`predictions` out of bound",
             "`weights` contains values that are not finite")


def _as_tensor(x):
    if isinstance(x, torch.Tensor):
        return x
    from .. import nn

    return torch.as_tensor(x, device=nn.device())


def remove_squeezable_dimensions(labels, predictions, expected_rank_diff=0, name=None):
    """squeeze the last dimension of the larger-rank argument when the ranks differ from `expected_rank_diff` by exactly one and that
    dimension is 1 (:13-62, the static-rank branch)"""
    labels, predictions = _as_tensor(labels), _as_tensor(predictions)
    rank_diff = predictions.dim() - labels.dim()
    if rank_diff == expected_rank_diff + 1 and predictions.shape[-1] == 1:
        predictions = predictions.squeeze(-1)
    elif rank_diff == expected_rank_diff - 1 and labels.shape[-1] == 1:
        labels = labels.squeeze(-1)
    return labels, predictions


def raise_for_counters(counters, what="confusion_matrix"):
    """the reference's assertions (:115-132) from the kernel's rejection counters [8] (one host read)"""
    c = [int(v) for v in counters.tolist()]
    for k, msg in enumerate(_MESSAGES):
        if c[k]:
            raise ValueError(f"{what}: {msg} ({c[k]} element{'s' if c[k] != 1 else ''})")
    return c


def prepare_weights(weights, shape, what):
    """-> (tensor for the kernel or None, w_exp): bool / uint8 as bytes, every other dtype as float32 with the fixed-point exponent"""
    if weights is None:
        return None, 0
    weights = _as_tensor(weights)
    if tuple(weights.shape) != tuple(shape):
        raise ValueError(f"{what}: `weights` must match `predictions` shape, got {tuple(weights.shape)} against {tuple(shape)}")
    if weights.dtype in (torch.bool, torch.uint8):
        return weights.contiguous(), 0
    w = weights.to(torch.float32).contiguous()
    m = K.confusion_absmax(w)
    if m != m or m == float("inf"):
        raise ValueError(f"{what}: {_MESSAGES[4]}")
    return w, K.confusion_weight_exponent(m)


def _num_classes(labels, predictions, num_classes, what):
    if num_classes is None:
        if labels.numel() == 0:
            return 0
        num_classes = int(torch.maximum(labels.max(), predictions.max()).item()) + 1
        if num_classes <= 0:
            raise ValueError(f"{what}: {_MESSAGES[0]}")
    num_classes = int(num_classes)
    if num_classes > 256:
        raise ValueError(f"{what}: num_classes = {num_classes}: at most 256 classes")
    return num_classes


def _batched(labels, predictions, num_classes, weights, dtype, what):
    """labels, predictions [B, n] int32 of one shape, weights None or [B, n] -> [B, C, C] of dtype"""
    C = _num_classes(labels, predictions, num_classes, what)
    B, n = labels.shape
    w, w_exp = prepare_weights(weights, labels.shape, what)
    if C == 0 or n == 0 or B == 0:
        return torch.zeros(B, C, C, dtype=dtype, device=labels.device)
    cm, counters = K.confusion_batched(labels.contiguous(), predictions.contiguous(), C, weights=w, w_exp=w_exp)
    raise_for_counters(counters, what)
    if w_exp == 0:
        return cm.to(dtype)
    return torch.ldexp(cm.double(), torch.tensor(-w_exp, device=cm.device)).to(dtype)


def confusion_matrix(labels, predictions, num_classes=None, weights=None, dtype=torch.int32, name=None):
    """[n, n] matrix, rows the real labels, columns the predictions, of two 1-D tensors of one shape (:65-143):
        confusion_matrix([1, 2, 4], [2, 2, 4]) ==> [[0 0 0 0 0] [0 0 1 0 0] [0 0 1 0 0] [0 0 0 0 0] [0 0 0 0 1]]
    num_classes None: one plus the largest value in either.  Values are cast to int32 (truncation, as tf.cast).  ValueError: mismatched
    shapes, a `weights` shape other than `predictions`', a negative or out-of-bound label or prediction (the reference's messages), a weight
    that is not finite.  See the module docstring for how weights are counted."""
    labels, predictions = remove_squeezable_dimensions(labels, predictions)
    if labels.dim() != 1 or tuple(labels.shape) != tuple(predictions.shape):
        raise ValueError(f"confusion_matrix: `labels` and `predictions` must be 1-D and of the same shape, got {tuple(labels.shape)} and "
                         f"{tuple(predictions.shape)}")
    if weights is not None and tuple(_as_tensor(weights).shape) != tuple(predictions.shape):
        raise ValueError(f"confusion_matrix: `weights` must match `predictions` shape, got {tuple(_as_tensor(weights).shape)}")
    K._require_cuda(labels, predictions)
    labels, predictions = labels.to(torch.int32).unsqueeze(0), predictions.to(torch.int32).unsqueeze(0)
    weights = None if weights is None else _as_tensor(weights).unsqueeze(0)
    return _batched(labels, predictions, num_classes, weights, dtype, "confusion_matrix")[0]


def batch_confusion_matrix(labels, predictions, num_classes=None, weights=None, dtype=torch.int32, name=None):
    """[B, n, n]: one matrix per sample of two tensors [B, ...] of one shape and rank >= 1, each sample flattened (:146-231).  Same casts,
    checks and weights as confusion_matrix."""
    labels, predictions = remove_squeezable_dimensions(labels, predictions)
    if tuple(labels.shape) != tuple(predictions.shape):
        raise ValueError(f"batch_confusion_matrix: `labels` and `predictions` must have the same shape, got {tuple(labels.shape)} and "
                         f"{tuple(predictions.shape)}")
    if labels.dim() < 1:
        raise ValueError("batch_confusion_matrix: `labels` and `predictions` must have rank >= 1 (batch first)")
    if weights is not None and tuple(_as_tensor(weights).shape) != tuple(predictions.shape):
        raise ValueError(f"batch_confusion_matrix: `weights` must match `predictions` shape, got {tuple(_as_tensor(weights).shape)}")
    K._require_cuda(labels, predictions)
    B = labels.shape[0]
    labels, predictions = labels.to(torch.int32).reshape(B, -1), predictions.to(torch.int32).reshape(B, -1)
    weights = None if weights is None else _as_tensor(weights).reshape(B, -1)
    return _batched(labels, predictions, num_classes, weights, dtype, "batch_confusion_matrix")
