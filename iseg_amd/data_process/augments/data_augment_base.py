"""Counterpart of the reference's augments/data_augment_base.py (:9-32).  Every augmentation here follows StandardAugmentationsPipeline's
split: the random decision is drawn on the host (`draw(height, width)`, from the object's own seeded numpy Generator) and the pixels are
moved on the device (`apply(image, label, decision)`); `call` is `apply(draw(...))`.  A sample is an image [H, W, 3] float32 (uint8
accepted) and a label [H, W, 1] or [H, W] int32 (or None), both on the device; the label keeps its rank."""
import numpy as np


class DataAugmentationBase:
    def __init__(self, name=None, seed=0):
        self.name = name or type(self).__name__
        self.rng = np.random.default_rng(seed)

    def __call__(self, *args, **kwargs):
        return self.call(*args, **kwargs)

    def draw(self, height, width):
        return None

    def apply(self, image, label, decision):
        return image, label

    def call(self, image, label=None):
        return self.apply(image, label, self.draw(int(image.shape[0]), int(image.shape[1])))


def executes(execute_prob, rng):
    """one draw: True with probability execute_prob, always at 1.0"""
    return bool(rng.random() <= execute_prob) or execute_prob == 1.0


def random_execute_helper(execute_prob, fn0, fn1, rng):
    """fn0() with probability execute_prob, else fn1()"""
    return (fn0 if executes(execute_prob, rng) else fn1)()
