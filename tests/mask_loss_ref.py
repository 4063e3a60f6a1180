"""fp64 restatement of the reference's MaskLoss (losses/mask_loss.py:10-201) on SegLossBase (losses/seg_loss_base.py:12-95) and of the Keras
loss wrapper's masked reduction, in plain torch so that gradients come from autograd.  Test infrastructure only.

    valid = y != ignore                     (before the ignore_label == 0 shift)
    t     = one_hot(y, C)                   zero row for every label outside [0, C)
    sigmoid term  mean_c[bce]  or  mean_c[(1 - p_t)^gamma * bce * w]    (keras binary_crossentropy / binary_focal_crossentropy, from_logits,
                                                                         logits form of tf.keras 2: bce = max(z,0) - z t + log1p(exp(-|z|)))
    dice term     1 - (2 sum(valid s t) + eps) / (sum(valid s) + sum(valid t) + eps)      per image, over classes and pixels
    CE term       -sum_c t log_softmax(z)  or keras categorical_focal_crossentropy (alpha 0.25, gamma 2, probabilities clipped to [eps, 1-eps])
    reduction=False -> sum(l * valid) / (sum(valid) + eps) ;  reduction=True -> l * valid, [B, HW]
"""
import torch

from oracle import tf_ops as O

EPS = 1e-7      # keras.backend.epsilon()


def dice(y_true, y_pred, from_logits=False, weighted_mask=None):
    """mask_loss.py:159-200: 1 - (2 sum(y_true y_pred) + eps) / (sum(y_true) + sum(y_pred) + eps), per leading index"""
    y_true = y_true.to(y_pred.dtype)
    if from_logits:
        y_pred = torch.sigmoid(y_pred)
    if weighted_mask is not None:
        w = weighted_mask.to(y_pred.dtype)
        y_pred = y_pred * w
        y_true = y_true * w
    B = y_pred.shape[0]
    a, b = y_true.reshape(B, -1), y_pred.reshape(B, -1)
    inter = 2.0 * (a * b).sum(-1) + EPS
    den = b.sum(-1) + a.sum(-1) + EPS
    return 1 - inter / den      # den >= eps > 0: divide_no_nan never takes its zero branch


def preprocess(y_true, y_pred, num_class, ignore_label):
    """-> labels at the logits' size (shifted when ignore_label == 0), valid [B, HW], one-hot t [B, HW, C]"""
    B, H, W, C = y_pred.shape
    y = y_true.to(torch.int64)
    if tuple(y.shape[1:3]) != (H, W):
        y = O.resize_nearest(y[..., None], (H, W))[..., 0]
    valid = (y != ignore_label).to(y_pred.dtype).reshape(B, -1)
    if ignore_label == 0:
        y = y - 1
    y = y.reshape(B, -1)
    inside = (y >= 0) & (y < num_class)
    t = torch.nn.functional.one_hot(torch.where(inside, y, torch.zeros_like(y)), num_class).to(y_pred.dtype) * inside[..., None].to(y_pred.dtype)
    return y, valid, t


def sigmoid_term(z, t, focal=True, class_balancing=False, alpha=0.25, gamma=2.0):
    """[B, HW, C] -> [B, HW]"""
    bce = torch.clamp(z, min=0) - z * t + torch.log1p(torch.exp(-z.abs()))
    if not focal:
        return bce.mean(-1)
    s = torch.sigmoid(z)
    p_t = t * s + (1 - t) * (1 - s)
    f = (1 - p_t) ** gamma * bce
    if class_balancing:
        f = f * (t * alpha + (1 - t) * (1 - alpha))
    return f.mean(-1)


def ce_term(z, t, focal=False, alpha=0.25, gamma=2.0):
    """[B, HW, C] -> [B, HW]"""
    if not focal:
        return -(t * torch.log_softmax(z, -1)).sum(-1)
    p = torch.softmax(z, -1)
    p = p / p.sum(-1, keepdim=True)
    p = torch.clamp(p, EPS, 1 - EPS)
    return (alpha * (1 - p) ** gamma * (-(t * torch.log(p)))).sum(-1)


def per_pixel(y_true, y_pred, num_class=21, ignore_label=255, use_sigmoid_loss=True, use_dice_loss=True, use_ce_loss=True,
              ce_loss_coefficient=1.0, sigmoid_loss_coefficient=20.0, dice_loss_coefficient=1.0, apply_focal_sigmoid_loss=True,
              apply_focal_ce_loss=False, apply_class_balancing=False):
    """compute_loss_forwards: (loss [B, HW] before the mask, valid [B, HW])"""
    B, H, W, C = y_pred.shape
    _, valid, t = preprocess(y_true, y_pred, num_class, ignore_label)
    z = y_pred.reshape(B, H * W, C)
    terms = []
    if use_sigmoid_loss:
        terms.append(sigmoid_loss_coefficient * sigmoid_term(z, t, apply_focal_sigmoid_loss, apply_class_balancing))
    if use_dice_loss:
        d = dice(t, z, from_logits=True, weighted_mask=valid[..., None])
        terms.append((dice_loss_coefficient * d)[:, None] + torch.zeros_like(valid))
    if use_ce_loss:
        terms.append(ce_loss_coefficient * ce_term(z, t, apply_focal_ce_loss))
    if not terms:
        raise ValueError("MaskLoss: no loss term enabled (tf.add_n of an empty list)")
    return sum(terms), valid


def mask_loss(y_true, y_pred, reduction=False, **kw):
    """the value the Keras loss wrapper returns: masked mean over the valid pixels, or the masked [B, HW] tensor when reduction=True"""
    loss, valid = per_pixel(y_true, y_pred, **kw)
    if reduction:
        return loss * valid
    return (loss * valid).sum() / (valid.sum() + EPS)
