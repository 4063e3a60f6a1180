"""data_process/ of the reference: input normalisation, the composable augmentations and the standard training recipe, on the device."""
from .input_norm import normalize_input_value_range, norm_affine  # noqa: F401
from .input_norm_types import InputNormTypes  # noqa: F401
from .mean_pixel import get_mean_pixel  # noqa: F401
from . import augments  # noqa: F401
from .augments import *  # noqa: F401,F403
from .pipeline import AugmentationsPipeLine, StandardAugmentationsPipeline  # noqa: F401
