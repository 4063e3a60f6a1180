"""losses/mask_loss.py of the reference (:10-201): MaskLoss, the Mask2Former-style sum of a per-class sigmoid (focal) loss, a per-image dice
loss and the softmax cross-entropy, with the ignore label carried as a Keras loss mask, and the module-level dice().

The loss and its gradient come from csrc/mask_loss.hip (two streaming passes over the logits, every flag combination on the same kernels).
`fused_mean` is the hook Trainer.train_step looks for: the masked mean and d(mean)/d(logits) from one call.  ISEG_MASKLOSS_FUSED=0 (read
per call) selects the composed route instead -- `compute_loss_forwards` below, built from the existing cross-entropy op and torch tensor
arithmetic on the device, reduced by SegLossBase.__call__ -- the A/B partner of the kernels.

`class_weights` is accepted and stored and, as in the reference, not used.  The focal sigmoid term is the logits form of tf.keras 2 (Keras 3
clips probabilities to [1e-7, 1 - 1e-7] instead: the same function for |z| < 16.1)."""
import os

import torch

from .. import functional as F
from .. import kernels as K
from .seg_loss_base import EPSILON, SegLossBase

_FOCAL_ALPHA, _FOCAL_GAMMA = 0.25, 2.0      # Keras defaults of binary_focal_crossentropy / categorical_focal_crossentropy


def _fused():
    return os.environ.get("ISEG_MASKLOSS_FUSED", "1") != "0"


class MaskLoss(SegLossBase):
    def __init__(self, num_class=21, ignore_label=255, batch_size=2, reduction=False, from_logits=True, class_weights=None,
                 use_sigmoid_loss=True, use_dice_loss=True, use_ce_loss=True, ce_loss_coefficient=1.0, sigmoid_loss_coefficient=20.0,
                 dice_loss_coefficient=1.0, apply_focal_sigmoid_loss=True, apply_focal_ce_loss=False, apply_class_balancing=False, name=None):
        super().__init__(num_class=num_class, ignore_label=ignore_label, batch_size=batch_size, reduction=reduction, from_logits=from_logits,
                         class_weights=class_weights, name=name)
        if not from_logits:
            raise NotImplementedError("from_logits=False is not used by the reference's training path")
        if not (use_sigmoid_loss or use_dice_loss or use_ce_loss):
            raise ValueError("MaskLoss: at least one of use_sigmoid_loss / use_dice_loss / use_ce_loss must be set (tf.add_n of an empty list)")
        self.use_sigmoid_loss = use_sigmoid_loss
        self.use_dice_loss = use_dice_loss
        self.use_ce_loss = use_ce_loss
        self.ce_loss_coefficient = ce_loss_coefficient
        self.sigmoid_loss_coefficient = sigmoid_loss_coefficient
        self.dice_loss_coefficient = dice_loss_coefficient
        self.apply_focal_sigmoid_loss = apply_focal_sigmoid_loss
        self.apply_focal_ce_loss = apply_focal_ce_loss
        self.apply_class_balancing = apply_class_balancing
        if self.reduction is None:
            self.fused_mean = None      # the trainer's hook is the scalar route only

    def _flags(self):
        return ((K.MASKLOSS_SIGMOID if self.use_sigmoid_loss else 0) | (K.MASKLOSS_DICE if self.use_dice_loss else 0) |
                (K.MASKLOSS_CE if self.use_ce_loss else 0) | (K.MASKLOSS_FOCAL_SIGMOID if self.apply_focal_sigmoid_loss else 0) |
                (K.MASKLOSS_FOCAL_CE if self.apply_focal_ce_loss else 0) | (K.MASKLOSS_CLASS_BALANCING if self.apply_class_balancing else 0))

    def _coefs(self):
        return (float(self.sigmoid_loss_coefficient), float(self.dice_loss_coefficient), float(self.ce_loss_coefficient))

    def _check(self, y_pred):
        if y_pred.dim() != 4 or y_pred.shape[-1] != self.num_class:
            raise ValueError(f"MaskLoss: y_pred must be [B, H, W, {self.num_class}], got {tuple(y_pred.shape)}")

    def __call__(self, y_true, y_pred):
        if not _fused():
            return super().__call__(y_true, y_pred)
        self._check(y_pred)
        y_true, y_pred, _ = self.internal_preprocess(y_true, y_pred)
        if self.reduction is None:
            return F.mask_loss_per_pixel(y_pred, y_true, self.ignore_label, self._flags(), self._coefs())
        return F.mask_loss_mean(y_pred, y_true, self.ignore_label, self._flags(), self._coefs(), 1.0)

    def fused_mean(self, y_true, y_pred, weight=1.0, cm=None):
        """weight * (masked mean over the valid pixels), differentiable; the gradient is computed with the loss"""
        if cm is not None:
            raise ValueError("MaskLoss has no confusion-matrix pass (confusion_spec is not set)")
        if not _fused():
            return SegLossBase.__call__(self, y_true, y_pred) * weight
        self._check(y_pred)
        y_true, y_pred, _ = self.internal_preprocess(y_true, y_pred)
        return F.mask_loss_mean(y_pred, y_true, self.ignore_label, self._flags(), self._coefs(), weight)

    def compute_loss_forwards(self, y_true, y_pred, valid_mask=None):
        """the composed route: per-pixel loss [B, H*W] (unmasked) with `_keras_mask` = valid_mask, as the reference's method returns it"""
        self._check(y_pred)
        batch_size, height, width, num_class = y_pred.shape
        labels = y_true - 1 if self.ignore_label == 0 else y_true
        labels = labels.reshape(batch_size, -1).to(torch.int64)
        inside = (labels >= 0) & (labels < num_class)
        y_true_one_hot = torch.nn.functional.one_hot(torch.where(inside, labels, torch.zeros_like(labels)), num_class).to(torch.float32)
        y_true_one_hot = y_true_one_hot * inside[..., None].to(torch.float32)      # [batch, h * w, num_class], zero row outside [0, C)
        z = y_pred.reshape(batch_size, height * width, num_class)
        loss_list = []
        if self.use_sigmoid_loss:
            bce = torch.clamp(z, min=0) - z * y_true_one_hot + torch.log1p(torch.exp(-z.abs()))
            if self.apply_focal_sigmoid_loss:
                s = torch.sigmoid(z)
                p_t = y_true_one_hot * s + (1 - y_true_one_hot) * (1 - s)
                bce = (1 - p_t) ** _FOCAL_GAMMA * bce
                if self.apply_class_balancing:
                    bce = bce * (y_true_one_hot * _FOCAL_ALPHA + (1 - y_true_one_hot) * (1 - _FOCAL_ALPHA))
            loss_list.append(bce.mean(-1) * self.sigmoid_loss_coefficient)
        if self.use_dice_loss:
            dice_loss = dice(y_true_one_hot, z, from_logits=True, weighted_mask=valid_mask[..., None])
            loss_list.append((dice_loss * self.dice_loss_coefficient)[:, None] + torch.zeros_like(valid_mask))
        if self.use_ce_loss:
            # the ignore-label cross-entropy op masks ignored pixels itself (they are masked again below) and shifts the labels itself
            focal = (_FOCAL_ALPHA, _FOCAL_GAMMA) if self.apply_focal_ce_loss else None
            ce_loss = F.softmax_ce_per_pixel(y_pred, y_true, num_class, self.ignore_label, None, focal)
            loss_list.append(ce_loss.reshape(batch_size, -1) * self.ce_loss_coefficient)
        loss = loss_list[0]
        for term in loss_list[1:]:
            loss = loss + term
        loss._keras_mask = valid_mask
        return loss


def dice(y_true, y_pred, from_logits=False, weighted_mask=None):
    """Computes the Dice loss value between `y_true` and `y_pred`, one value per leading (batch) index.

    Formula:
        loss = 1 - (2 * sum(y_true * y_pred)) / (sum(y_true) + sum(y_pred))
    (keras.backend.epsilon() joins numerator and denominator, mask_loss.py:190-194)"""
    y_true = y_true.to(y_pred.dtype)
    batch_size = y_pred.shape[0]
    if from_logits:
        y_pred = torch.sigmoid(y_pred)
    if weighted_mask is not None:
        weighted_mask = weighted_mask.to(y_pred.dtype)
        y_pred = y_pred * weighted_mask
        y_true = y_true * weighted_mask
    inputs = y_true.reshape(batch_size, -1)
    targets = y_pred.reshape(batch_size, -1)
    intersection = (inputs * targets).sum(-1) * 2.0 + EPSILON
    den = targets.sum(-1) + inputs.sum(-1) + EPSILON
    ratio = torch.where(den == 0, torch.zeros_like(den), intersection / den)      # tf.math.divide_no_nan
    return 1 - ratio
