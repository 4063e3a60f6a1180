"""Counterpart of the reference's augments/pad_augment.py (:12-59): pad bottom / right up to (target_height, target_width) with image_pad_value /
label_pad_value; a sample that is already larger keeps its size."""
from ._gather import gather
from .data_augment_base import DataAugmentationBase


class PadAugment(DataAugmentationBase):
    def __init__(self, target_height, target_width, image_pad_value=[127.5, 127.5, 127.5], label_pad_value=255, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.target_height, self.target_width = target_height, target_width
        self.image_pad_value, self.label_pad_value = image_pad_value, label_pad_value

    def draw(self, height, width):
        """the padded size"""
        return height + max(self.target_height - height, 0), width + max(self.target_width - width, 0)

    def apply(self, image, label, decision):
        return gather(image, label, out_size=decision, pad_value=self.image_pad_value, pad_label=self.label_pad_value)
