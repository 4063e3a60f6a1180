"""What the photometric classes share: one launch of the gather kernel with the float table's slot(s) set, or the device clip alone.

DEPARTURE FROM THE REFERENCE: the gather kernel ends every contrast / saturation / hue step with a clip to [0, 256] -- the clip
RandomPhotoMetricDistortions applies once at its end.  The reference's stand-alone RandomContrastAugment and RandomSaturationAugment do not
clip, so there a strong contrast factor can leave values below 0 or above 256 for a later stage to see; here it cannot.  The results agree
whenever the unclipped value stays inside [0, 256], and always for RandomPhotoMetricDistortions.call / contrast_first_forward (whose last
stage, hue, clips in the reference as well).  contrast_last_forward clips after its contrast stage, which the reference leaves unclipped.
tests/test_augments_gpu.py pins this (test_stand_alone_contrast_clips_where_the_reference_does_not)."""
import torch

from ... import kernels as K
from ._gather import gather, image_tensor


def clip_pixels(image):
    """tf.clip_by_value(image, 0, 256) on the device"""
    return K.clip_fwd(image_tensor(image).to(torch.float32).contiguous(), 0.0, 256.0)


def adjust(image, label, slots):
    """slots: {float-table slot: value}; values equal to the slot's identity are left out by the callers"""
    return gather(image, None, photometric=slots)[0], label
