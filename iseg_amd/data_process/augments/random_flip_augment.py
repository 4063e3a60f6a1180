"""Counterpart of the reference's augments/random_flip_augment.py (:12-41): left-right flip with probability prob_of_flip; `reversed_label`, when given,
replaces the label of a flipped sample instead of being flipped."""
from ._gather import gather
from .data_augment_base import DataAugmentationBase


class RandomFlipAugment(DataAugmentationBase):
    def __init__(self, prob_of_flip=0.5, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.prob_of_flip = prob_of_flip

    def draw(self, height, width):
        return bool(self.rng.random() <= self.prob_of_flip)

    def apply(self, image, label, decision, reversed_label=None):
        if not decision:
            return image, label
        return self._execute_branch(image, label, reversed_label)

    def call(self, image, label, reversed_label=None):
        return self.apply(image, label, self.draw(int(image.shape[0]), int(image.shape[1])), reversed_label)

    def _execute_branch(self, image, label, reversed_label):
        if label is not None and reversed_label is not None:
            return gather(image, None, flip=True)[0], reversed_label
        return gather(image, label, flip=True)
