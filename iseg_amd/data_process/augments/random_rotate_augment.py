"""Counterpart of the reference's augments/random_rotate_augment.py (:20-296): rotation by a uniform angle in [0, 2 pi) about the image centre as ONE
projective transform on the device (csrc/projective.hip): the image bilinear with a fill of -1 and then where(out < -1e-6,
fill_constant_color, out), the label nearest with a fill of ignore_label, both from the same matrix.  The matrix is built on the host in
float32 numpy with the reference's formulas, so the kernel receives the very numbers a test (or the reference) computes."""
import numpy as np
import torch

from ... import kernels as K
from .data_augment_base import DataAugmentationBase


def _transforms_on(device, transforms, batch):
    t = transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else np.asarray(transforms)
    t = np.broadcast_to(t.astype(np.float32).reshape(-1, 8), (batch, 8)).copy()
    return torch.from_numpy(t).to(device)


def transform(images, transforms, fill_mode="reflect", fill_value=0.0, interpolation="bilinear", output_shape=None, name=None):
    """tf.raw_ops.ImageProjectiveTransformV3 (:20-115) for images [N, H, W, C] (C in 1..4) on the device and transforms [8] or [N, 8]
    (a0 a1 a2 b0 b1 b2 c0 c1: output (x, y) -> input ((a0 x + a1 y + a2) / k, (b0 x + b1 y + b2) / k), k = c0 x + c1 y + 1).  Only what the
    reference uses: fill_mode "constant" and the input's own size as output_shape.  The result is float32 whatever the input's type."""
    if fill_mode.lower() != "constant":
        raise NotImplementedError(f"fill_mode {fill_mode!r}: only 'constant' is implemented on the device (the reference uses no other)")
    if interpolation.lower() not in ("nearest", "bilinear"):
        raise ValueError(f"interpolation must be 'nearest' or 'bilinear', got {interpolation!r}")
    if images.dim() != 4:
        raise ValueError(f"images must be [N, H, W, C], got {tuple(images.shape)}")
    if output_shape is not None and tuple(int(v) for v in output_shape) != (int(images.shape[1]), int(images.shape[2])):
        raise NotImplementedError("output_shape different from the input's size is not implemented (the reference never passes one)")
    out, _ = K.projective_transform_batch(images, None, _transforms_on(images.device, transforms, int(images.shape[0])),
                                          interpolation=interpolation.lower(), image_fill=float(fill_value))
    return out


def get_rotation_matrix(angles, image_height, image_width, name=None):
    """[N, 8] float32 projective transforms of a rotation by angles [N] about the centre of an image_height x image_width image (:118-167),
    on the host; image_height / image_width may be one number or one per angle"""
    f = np.float32
    angles = np.atleast_1d(np.asarray(angles, dtype=f))
    image_height = np.asarray(image_height, dtype=f)
    image_width = np.asarray(image_width, dtype=f)
    cos, sin = np.cos(angles).astype(f), np.sin(angles).astype(f)
    x_offset = ((image_width - f(1)) - (cos * (image_width - f(1)) - sin * (image_height - f(1)))) / f(2.0)
    y_offset = ((image_height - f(1)) - (sin * (image_width - f(1)) + cos * (image_height - f(1)))) / f(2.0)
    zeros = np.zeros_like(angles)
    return np.stack([cos, -sin, x_offset.astype(f), sin, cos, y_offset.astype(f), zeros, zeros], axis=1).astype(f)


class RandomRotateAugment(DataAugmentationBase):
    def __init__(self, prob_of_rotate=0.5, fill_constant_color=[0, 0, 0], ignore_label=255, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.prob_of_rotate, self.fill_constant_color, self.ignore_label = prob_of_rotate, fill_constant_color, ignore_label

    def draw(self, height, width):
        """the angle (float32, [0, 2 pi)), or None when the sample is not rotated"""
        if self.rng.random() <= self.prob_of_rotate:
            return self.draw_angles(1)[0]
        return None

    def draw_angles(self, n, lower=0.0, upper=1.0):
        return self.rng.uniform(lower * 2.0 * np.pi, upper * 2.0 * np.pi, size=n).astype(np.float32)

    def apply(self, image, label, decision):
        if decision is None:
            return image, label
        return self.rotate(image, label, np.asarray([decision], dtype=np.float32))

    def _execute_branch(self, image, label):
        return self.random_rotated_inputs(image, labels=label) if label is not None else (self.random_rotated_inputs(image), None)

    def random_rotated_inputs(self, images, labels=None, lower=0.0, upper=1.0):
        """images [H, W, 3] or [N, H, W, 3], one angle in [lower, upper) turns per batch entry (:221-296)"""
        batch = 1 if images.dim() == 3 else int(images.shape[0])
        output_images, output_labels = self.rotate(images, labels, self.draw_angles(batch, lower, upper))
        return (output_images, output_labels) if labels is not None else output_images

    def rotate(self, images, labels, angles):
        """rank 3 or rank 4 images (labels with or without the channel axis) by the given angles, every sample about the buffer's centre"""
        unbatched = images.dim() == 3
        if unbatched:
            images = images[None]
            labels = None if labels is None else labels[None]
        if images.dim() != 4:
            raise ValueError(f"images must be [H, W, C] or [N, H, W, C], got {tuple(images.shape)}")
        out, out_lab = self.apply_batch(images, labels, None, angles)
        if unbatched:
            out = out[0]
            out_lab = None if out_lab is None else out_lab[0]
        return out, out_lab

    def apply_batch(self, images, labels, sizes, angles):
        """one launch for a padded batch: images [B, Hs, Ws, 3], labels [B, Hs, Ws] or [B, Hs, Ws, 1] int32 or None, sizes [(H, W), ...] of
        the samples in the top-left corners of their slots (None = all Hs x Ws), angles [B]; every sample turns about its OWN centre.  The
        padding of the buffer comes back as fill_constant_color / ignore_label."""
        if images.dim() != 4 or images.shape[-1] != len(self.fill_constant_color):
            raise ValueError(f"images must be [B, Hs, Ws, {len(self.fill_constant_color)}] (one fill_constant_color value per channel), "
                             f"got {tuple(images.shape)}")
        B, Hs, Ws, _ = images.shape
        angles = np.asarray(angles, dtype=np.float32).reshape(-1)
        if angles.shape[0] != B:
            raise ValueError(f"one angle per batch entry: {B} entries, {angles.shape[0]} angles")
        sdev = None
        if sizes is None:
            matrix = get_rotation_matrix(angles, Hs, Ws)
        else:
            s = np.asarray(sizes, dtype=np.int32).reshape(B, 2)
            if (s < 0).any() or (s[:, 0] > Hs).any() or (s[:, 1] > Ws).any():
                raise ValueError("sizes must lie inside the padded buffer")
            matrix = get_rotation_matrix(angles, s[:, 0], s[:, 1])
            sdev = torch.from_numpy(s).to(images.device)
        channel_axis = labels is not None and labels.dim() == 4
        lab = labels[..., 0] if channel_axis else labels
        out, out_lab = K.projective_transform_batch(images, lab, torch.from_numpy(matrix).to(images.device), sizes=sdev,
                                                    interpolation="bilinear", image_fill=-1.0,
                                                    replace=[float(v) for v in self.fill_constant_color], label_fill=int(self.ignore_label))
        if channel_axis:
            out_lab = out_lab[..., None]
        return out, out_lab
