"""data_process/augments/ of the reference: the composable augmentations, one file per class under the reference's file names.  Decisions
are drawn on the host, pixels move on the device (data_augment_base.py)."""
from .data_augment_base import DataAugmentationBase, random_execute_helper  # noqa: F401
from .resize_augment import ResizeAugment  # noqa: F401
from .random_scale_augment import RandomScaleAugment  # noqa: F401
from .pad_augment import PadAugment  # noqa: F401
from .pad_to_odd_augment import PadToOddAugment, pad_to_odd  # noqa: F401
from .random_crop_augment import RandomCropAugment  # noqa: F401
from .random_flip_augment import RandomFlipAugment  # noqa: F401
from .random_brightness_augment import RandomBrightnessAugment  # noqa: F401
from .random_contrast_augment import RandomContrastAugment  # noqa: F401
from .random_hue_augment import RandomHueAugment  # noqa: F401
from .random_saturation_augment import RandomSaturationAugment  # noqa: F401
from .random_photo_metric_distortions import RandomPhotoMetricDistortions  # noqa: F401
from .random_erasing_augment import RandomErasingAugment  # noqa: F401
from .random_jepg_quality_augment import RandomJEPGQualityAugment  # noqa: F401
from .random_noisy_eval_augment import RandomNoisyEvalAugment  # noqa: F401
from .random_rotate_augment import RandomRotateAugment  # noqa: F401
from .lambda_augment import LambdaAugment  # noqa: F401

__all__ = ["DataAugmentationBase", "ResizeAugment", "RandomScaleAugment", "PadAugment", "PadToOddAugment", "RandomCropAugment",
           "RandomFlipAugment", "RandomBrightnessAugment", "RandomContrastAugment", "RandomHueAugment", "RandomSaturationAugment",
           "RandomPhotoMetricDistortions", "RandomErasingAugment", "RandomJEPGQualityAugment", "RandomNoisyEvalAugment",
           "RandomRotateAugment", "LambdaAugment"]
