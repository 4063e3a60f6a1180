"""Counterpart of the reference's augments/resize_augment.py (:13-70): bound a sample by (max_resize_height, max_resize_width), aspect kept, never larger
than it was; bilinear image / nearest label through the device resize kernels."""
import numpy as np
import torch

from ... import kernels as K
from ._gather import image_tensor, join_label, split_label
from .data_augment_base import DataAugmentationBase


def resize_image_and_label(image, label, height, width):
    """tf.image.resize of one sample: K.resize_bilinear / K.resize_nearest_i32"""
    image = image_tensor(image).to(torch.float32)
    if (height, width) == (int(image.shape[0]), int(image.shape[1])):
        return image, label
    lab2d, rank = split_label(label)
    out = K.resize_bilinear(image[None].contiguous(), height, width)[0]
    if lab2d is not None:
        lab2d = K.resize_nearest_i32(lab2d[None, :, :, None].contiguous(), height, width)[0, :, :, 0]
    return out, join_label(lab2d, rank)


class ResizeAugment(DataAugmentationBase):
    def __init__(self, max_resize_height, max_resize_width, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.max_resize_height, self.max_resize_width = max_resize_height, max_resize_width

    def compuate_target_size(self, height, width):
        """(:22-42) in its float32 arithmetic"""
        f = np.float32
        target_height = min(int(self.max_resize_height), height)
        target_width = int(f(width) * f(target_height) / f(height))
        target_width = min(int(self.max_resize_width), target_width)
        target_width = min(width, target_width)
        target_height = int(f(height) * f(target_width) / f(width))
        return target_height, target_width

    def draw(self, height, width):
        return self.compuate_target_size(height, width)

    def apply(self, image, label, decision):
        return resize_image_and_label(image, label, int(decision[0]), int(decision[1]))
