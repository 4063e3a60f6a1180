"""Counterpart of the reference's augments/random_photo_metric_distortions.py (:14-46): contrast U[0.75, 1.25) p 0.5 -> saturation
U[0.75, 1.25) p 0.5 -> hue U[-0.1, 0.1) always -> clip [0, 256], as ONE launch of the gather kernel (the three share its float table)."""
from ._photometric import adjust, clip_pixels
from .data_augment_base import DataAugmentationBase
from .random_contrast_augment import RandomContrastAugment
from .random_hue_augment import RandomHueAugment
from .random_saturation_augment import RandomSaturationAugment

_SLOT = {"random_contrast": (1, 1.0), "random_saturation": (5, 1.0), "random_hue": (6, 0.0)}      # stage -> (float-table slot, identity)


class RandomPhotoMetricDistortions(DataAugmentationBase):
    def __init__(self, name=None, seed=0):
        super().__init__(name=name, seed=seed)
        stages = {"random_contrast": RandomContrastAugment(0.75, 1.25, execute_prob=0.5),
                  "random_saturation": RandomSaturationAugment(0.75, 1.25, execute_prob=0.5),
                  "random_hue": RandomHueAugment(0.1, execute_prob=1.0)}
        for attr, stage in stages.items():      # public under the reference's attribute names; one random stream for the three
            stage.rng = self.rng
            setattr(self, attr, stage)

    def _draw(self, order, height, width):
        return {attr: getattr(self, attr).draw(height, width) for attr in order}

    def draw(self, height, width):
        """(contrast factor or None, saturation factor or None, hue delta), drawn in this order"""
        return tuple(self._draw(("random_contrast", "random_saturation", "random_hue"), height, width).values())

    def _launch(self, image, label, values):
        slots = {_SLOT[attr][0]: v for attr, v in values.items() if v is not None and v != _SLOT[attr][1]}
        return adjust(image, label, slots) if slots else (clip_pixels(image), label)

    def apply(self, image, label, decision):
        return self._launch(image, label, dict(zip(("random_contrast", "random_saturation", "random_hue"), decision)))

    def contrast_first_forward(self, image, label):
        """contrast -> saturation -> hue: the gather kernel's own order, one launch (the hue stage of the reference ends with the clip)"""
        return self.apply(image, label, self.draw(int(image.shape[0]), int(image.shape[1])))

    def contrast_last_forward(self, image, label):
        """saturation -> hue in one launch, then contrast in a second one; both end with the device step's clip to [0, 256], where the
        reference leaves the contrast result unclipped (_photometric.py)"""
        drawn = self._draw(("random_saturation", "random_hue", "random_contrast"), int(image.shape[0]), int(image.shape[1]))
        image, label = self._launch(image, label, {k: drawn[k] for k in ("random_saturation", "random_hue")})
        return self.random_contrast.apply(image, label, drawn["random_contrast"])
