"""Counterpart of the reference's augments/random_jepg_quality_augment.py (:11-27): a JPEG codec round trip at a random quality.  Constructible, so that
a recipe that lists it imports; not part of the on-device pipeline."""
from .data_augment_base import DataAugmentationBase


class RandomJEPGQualityAugment(DataAugmentationBase):
    def __init__(self, name=None, seed=0):
        super().__init__(name=name, seed=seed)

    def call(self, image, label=None):
        raise NotImplementedError("RandomJEPGQualityAugment (a JPEG codec round trip) is not part of the on-device pipeline "
                                  "(the standard recipe leaves it off)")
