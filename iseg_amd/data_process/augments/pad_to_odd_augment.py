"""Counterpart of the reference's augments/pad_to_odd_augment.py (:12-41): one more row / column where the height / width is even."""
from ._gather import gather
from .data_augment_base import DataAugmentationBase


def pad_to_odd(image, label=None, image_pad_value=[127.5, 127.5, 127.5], label_pad_value=255):
    height, width = int(image.shape[0]), int(image.shape[1])
    return gather(image, label, out_size=(height + int(height % 2 == 0), width + int(width % 2 == 0)), pad_value=image_pad_value,
                  pad_label=label_pad_value)


class PadToOddAugment(DataAugmentationBase):
    def __init__(self, image_pad_value=[127.5, 127.5, 127.5], label_pad_value=255, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.image_pad_value, self.label_pad_value = image_pad_value, label_pad_value

    def draw(self, height, width):
        return height + int(height % 2 == 0), width + int(width % 2 == 0)

    def apply(self, image, label, decision):
        return gather(image, label, out_size=decision, pad_value=self.image_pad_value, pad_label=self.label_pad_value)
