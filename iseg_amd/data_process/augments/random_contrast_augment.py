"""Counterpart of the reference's augments/random_contrast_augment.py (:12-28): with probability execute_prob, tf.image.random_contrast = (x - mean) *
U[lower, upper) + mean about each channel's mean over the image (K.augment_channel_means).  The device step ends with a clip to [0, 256]
(_photometric.py)."""
from ._photometric import adjust
from .data_augment_base import DataAugmentationBase, executes


class RandomContrastAugment(DataAugmentationBase):
    def __init__(self, lower=0.5, upper=1.5, execute_prob=0.5, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.lower, self.upper, self.execute_prob = lower, upper, execute_prob

    def draw(self, height, width):
        """the factor, or None when not executed"""
        if executes(self.execute_prob, self.rng):
            return float(self.rng.uniform(self.lower, self.upper))
        return None

    def apply(self, image, label, decision):
        if decision is None or decision == 1.0:
            return image, label
        return adjust(image, label, {1: decision})
