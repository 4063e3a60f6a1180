"""Counterpart of the reference's augments/random_hue_augment.py (:12-28): with probability execute_prob, tf.image.random_hue = H + U[-max_delta,
max_delta) in HSV; clip to [0, 256] either way."""
from ._photometric import adjust, clip_pixels
from .data_augment_base import DataAugmentationBase, executes


class RandomHueAugment(DataAugmentationBase):
    def __init__(self, max_delta=0.1, execute_prob=0.5, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.max_delta, self.execute_prob = max_delta, execute_prob

    def draw(self, height, width):
        """the delta, or None when not executed"""
        if executes(self.execute_prob, self.rng):
            return float(self.rng.uniform(-self.max_delta, self.max_delta))
        return None

    def apply(self, image, label, decision):
        if decision is None or decision == 0.0:
            return clip_pixels(image), label
        return adjust(image, label, {6: decision})
