"""Counterpart of the reference's augments/random_erasing_augment.py (:12-134): with probability `prob`, min_area_count .. max_area_count - 1 rectangles of
up to max_area_size of each side are filled with fill_constant_color (or uniform noise in [0, 255)) and their labels set to ignore_label.
The noise fill is the gather kernel's erase stage (its noise is drawn on the device from the seed in the decision); the constant fill is a
strided fill of the rectangle, pure data movement."""
import numpy as np
import torch

from ._gather import MAX_RECTS, gather, image_tensor
from .data_augment_base import DataAugmentationBase, executes


class RandomErasingAugment(DataAugmentationBase):
    def __init__(self, prob=0.25, min_area_size=0, max_area_size=0.25, min_area_count=1, max_area_count=3, fill_constant_color=[0, 0, 0],
                 use_fill_noise_color=False, ignore_label=255, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        self.min_area_size, self.max_area_size = float(min_area_size), float(max_area_size)
        if not 0.0 <= self.min_area_size <= self.max_area_size <= 1.0:
            raise ValueError(f"area sizes are fractions of a side with 0 <= min <= max <= 1, got {min_area_size}, {max_area_size}")
        self.prob, self.ignore_label, self.use_fill_noise_color = prob, ignore_label, use_fill_noise_color
        self.min_area_count, self.max_area_count = min_area_count, max_area_count
        # one grey value or one value per channel; None = black
        self._fill_constant_color = [float(v) for v in np.atleast_1d([0, 0, 0] if fill_constant_color is None else fill_constant_color)]
        if len(self._fill_constant_color) not in (1, 3):
            raise ValueError(f"fill_constant_color takes 1 or 3 values, got {fill_constant_color}")

    def _uniform_int(self, lo, hi):
        """an integer in [lo, hi); an empty range gives lo"""
        return int(self.rng.integers(lo, max(hi, lo + 1)))

    def draw(self, height, width):
        """None (not executed) or {"rects": [(y, x, h, w), ...], "seed": noise seed}: min_area_count .. max_area_count - 1 rectangles, each
        side between the min and max fraction of the image's (computed in float32 and truncated, at least one pixel), placed uniformly where
        they fit"""
        if not executes(self.prob, self.rng):
            return None
        sides = [(int(np.float32(n) * np.float32(self.min_area_size)), int(np.float32(n) * np.float32(self.max_area_size)))
                 for n in (height, width)]
        rects = []
        for _ in range(min(self._uniform_int(self.min_area_count, self.max_area_count), self.max_area_count)):
            ah, aw = (min(max(self._uniform_int(lo, hi), 1), n) for (lo, hi), n in zip(sides, (height, width)))
            rects.append((self._uniform_int(0, height - ah), self._uniform_int(0, width - aw), ah, aw))
        return {"rects": rects, "seed": int(self.rng.integers(0, 2 ** 63))}

    def apply(self, image, label, decision):
        if decision is None or not decision["rects"]:
            return image, label
        rects = decision["rects"]
        if self.use_fill_noise_color:
            for e in range(0, len(rects), MAX_RECTS):      # in drawing order: a later rectangle overwrites an earlier one
                image, label = gather(image, label, rects=rects[e:e + MAX_RECTS], pad_label=self.ignore_label, seed=decision["seed"] + e)
            return image, label
        image = image_tensor(image).clone()
        label = None if label is None else label.clone()
        fill = torch.tensor(self._fill_constant_color * (3 // len(self._fill_constant_color)), dtype=torch.float32)
        fill = fill.to(device=image.device, dtype=image.dtype)
        for y, x, h, w in rects:
            image[y:y + h, x:x + w] = fill
            if label is not None:
                label[y:y + h, x:x + w] = self.ignore_label
        return image, label
