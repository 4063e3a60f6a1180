"""Counterpart of the reference's augments/lambda_augment.py (:12-20): any callable as a pipeline stage."""
from .data_augment_base import DataAugmentationBase


class LambdaAugment(DataAugmentationBase):
    def __init__(self, fn, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.fn = fn

    def call(self, *args):
        return self.fn(*args)
