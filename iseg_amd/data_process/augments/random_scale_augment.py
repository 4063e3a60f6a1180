"""Counterpart of the reference's augments/random_scale_augment.py (:12-52) with utils.py:303-370: one of the discrete factors min..max step (step 0 =
continuous), optionally a neighbouring factor per axis (break_aspect_ratio); bilinear image / nearest label."""
import numpy as np

from .data_augment_base import DataAugmentationBase
from .resize_augment import resize_image_and_label


class RandomScaleAugment(DataAugmentationBase):
    def __init__(self, min_scale_factor=0.5, max_scale_factor=2.0, scale_factor_step_size=0.1, break_aspect_ratio=False, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.min_scale_factor, self.max_scale_factor = min_scale_factor, max_scale_factor
        self.scale_factor_step_size, self.break_aspect_ratio = scale_factor_step_size, break_aspect_ratio

    def get_random_scale(self):
        """utils.py:303-328"""
        lo, hi, step = self.min_scale_factor, self.max_scale_factor, self.scale_factor_step_size
        if lo < 0 or lo > hi:
            raise ValueError("Unexpected value of min_scale_factor.")
        if lo == hi:
            return float(lo)
        if step == 0:
            return float(self.rng.uniform(lo, hi))
        num_steps = int((hi - lo) / step + 1)
        return float(np.linspace(np.float32(lo), np.float32(hi), num_steps, dtype=np.float32)[self.rng.integers(0, num_steps)])

    def draw(self, height, width):
        """(scale_h, scale_w)"""
        scale_h = self.get_random_scale()
        if not self.break_aspect_ratio:
            return scale_h, scale_h
        scale_list = [scale_h - self.scale_factor_step_size, scale_h, scale_h + self.scale_factor_step_size]
        scale_h, scale_w = (float(np.clip(scale_list[self.rng.integers(0, 3)], self.min_scale_factor, self.max_scale_factor)) for _ in range(2))
        return scale_h, scale_w

    def apply(self, image, label, decision):
        scale_h, scale_w = decision
        if scale_h == 1.0 and scale_w == 1.0:
            return image, label
        # tf.cast(tf.cast(h, float32) * scale, int32)
        new_height = int(np.float32(image.shape[0]) * np.float32(scale_h))
        new_width = int(np.float32(image.shape[1]) * np.float32(scale_w))
        return resize_image_and_label(image, label, new_height, new_width)
