"""Counterpart of the reference's augments/random_noisy_eval_augment.py (:11-31): + N(0, noise_level) per pixel and channel, clip [0, 256]; a level of
1e-3 or less does nothing.  The noise is drawn on the device from the seed in the decision."""
from ._gather import gather
from .data_augment_base import DataAugmentationBase


class RandomNoisyEvalAugment(DataAugmentationBase):
    def __init__(self, noise_level=0, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.noise_level = noise_level

    def draw(self, height, width):
        """the noise seed, or None when the level is off"""
        if self.noise_level <= 0 + 1e-3:
            return None
        return int(self.rng.integers(0, 2 ** 63))

    def apply(self, image, label, decision):
        if decision is None:
            return image, label
        return gather(image, None, photometric={7: float(self.noise_level)}, seed=decision)[0], label
