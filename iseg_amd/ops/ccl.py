"""Connected-components labelling (ops/ccl.py of the reference) on csrc/ccl.hip.

The reference is a serial flood fill written for XLA; this one is a union-find over pixels in six launches (kernels.ccl_label).  Same result:
background 0, 4-connected components numbered 1, 2, 3, ... in the raster order of their first pixel, image by image.  Any non-zero value is
foreground, and uint8 / bool masks are taken as well as int32 (the reference negates a pixel that is neither 0 nor 1).  No gradient.
"""
from .. import kernels as K


def label_components(binary_img, return_counts=False):
    """binary_img [N,H,W] (or [H,W]) int32 / uint8 / bool on the device -> labels int32 of the same shape; with return_counts also the
    components per image, [N] int32 (= labels.amax((1, 2)))"""
    labels, counts = K.ccl_label(binary_img)
    return (labels, counts) if return_counts else labels
