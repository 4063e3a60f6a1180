"""losses/seg_loss_base.py of the reference (:12-95): SegLossBase, a keras.losses.Loss whose subclasses return the per-pixel loss [B, H*W]
with the ignore label attached as a Keras loss mask (`loss._keras_mask`).

Keras' loss wrapper then applies the mask and reduces; `__call__` restates that here:
    reduction=False (-> "sum_over_batch_size"):  sum(loss * mask) / (sum(mask) + 1e-7)      a mean over the VALID pixels
    reduction=True  (-> none):                   loss * mask, [B, H*W]
All arithmetic is fp32 (get_stable_float_dtype_for_loss() of the reference returns tf.float32)."""
import torch

from .. import kernels as K

EPSILON = 1e-7      # keras.backend.epsilon()


class SegLossBase:
    def __init__(self, num_class=21, ignore_label=255, batch_size=2, reduction=False, from_logits=True, class_weights=None, name=None):
        if isinstance(reduction, bool):
            reduction = "sum_over_batch_size" if not reduction else None
        self.reduction = reduction
        self.name = name
        self.num_class = num_class
        self.ignore_label = ignore_label
        self.batch_size = batch_size
        self.from_logits = from_logits
        self.class_weights = class_weights

    def __call__(self, y_true, y_pred):
        loss = self.call(y_true, y_pred)
        mask = getattr(loss, "_keras_mask", None)
        if mask is not None:
            loss = loss * mask
        if self.reduction is None:
            return loss
        if mask is None:
            return loss.mean()
        return loss.sum() / (mask.sum() + EPSILON)

    def call(self, y_true, y_pred):
        return self.internal_call(y_true, y_pred)

    def internal_call(self, y_true, y_pred):
        y_true, y_pred, valid_mask = self.internal_preprocess(y_true, y_pred)
        return self.compute_loss_forwards(y_true, y_pred, valid_mask=valid_mask)

    def internal_preprocess(self, y_true, y_pred):
        """labels int32 [B, h, w] nearest-resized to the logits' size, logits fp32 [B, H, W, C], valid mask fp32 [B, H*W]"""
        y_true = y_true.to(torch.int32)
        if y_pred.dtype != torch.float32:
            y_pred = K.cast(y_pred.contiguous(), torch.float32)
        _, height, width, _ = y_pred.shape
        if tuple(y_true.shape[1:3]) != (height, width):
            y_true = K.resize_nearest_i32(y_true.contiguous()[..., None], height, width)[..., 0]
        valid_mask = self.compute_valid_mask(y_true, dtype=torch.float32)
        y_true, y_pred = self.before_compute_loss_forward(y_true, y_pred)
        return y_true, y_pred, valid_mask

    def compute_valid_mask(self, y_true, dtype=None):
        dtype = dtype if dtype is not None else y_true.dtype
        return (y_true != self.ignore_label).to(dtype).reshape(y_true.shape[0], -1)

    def before_compute_loss_forward(self, y_true, y_pred):
        return y_true, y_pred

    def compute_loss_forwards(self, y_true, y_pred, valid_mask=None):
        raise NotImplementedError("compute_loss_forwards() is not implemented.")
