"""Counterpart of the reference's augments/random_crop_augment.py (:12-28) with utils.py:64-138 random_crop: one uniform offset for image and label."""
from ._gather import gather
from .data_augment_base import DataAugmentationBase


class RandomCropAugment(DataAugmentationBase):
    def __init__(self, crop_height=513, crop_width=513, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.crop_height, self.crop_width = crop_height, crop_width

    def draw(self, height, width):
        """(offset_height, offset_width), uniform over the positions at which the window fits"""
        if height < self.crop_height or width < self.crop_width:
            raise ValueError("Crop size greater than the image size.")
        return int(self.rng.integers(0, height - self.crop_height + 1)), int(self.rng.integers(0, width - self.crop_width + 1))

    def apply(self, image, label, decision):
        oy, ox = int(decision[0]), int(decision[1])
        if oy < 0 or ox < 0 or oy + self.crop_height > image.shape[0] or ox + self.crop_width > image.shape[1]:
            raise ValueError("Crop size greater than the image size.")
        return gather(image, label, out_size=(self.crop_height, self.crop_width), offset=(oy, ox))
