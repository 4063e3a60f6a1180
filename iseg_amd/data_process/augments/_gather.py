"""One sample through csrc/augment.hip's gather (K.augment_crop_batch) with a parameter table that is the identity for every stage the
caller does not ask for: no scale, offset 0, no flip, no erase rectangle, no photometric value, norm_scale 1 and norm_shift 0.  The table
layout is StandardAugmentationsPipeline.draw / draw_photometric's."""
import numpy as np
import torch

from ... import kernels as K

MAX_RECTS = 5      # erase rectangles one launch of the gather kernel takes


def split_label(label):
    """label [H, W, 1] / [H, W] / None -> ([H, W] int32 or None, rank)"""
    if label is None:
        return None, 0
    if label.dim() == 3:
        if label.shape[-1] != 1:
            raise ValueError(f"label must be [H, W, 1] or [H, W], got {tuple(label.shape)}")
        return label[:, :, 0].to(torch.int32), 3
    if label.dim() != 2:
        raise ValueError(f"label must be [H, W, 1] or [H, W], got {tuple(label.shape)}")
    return label.to(torch.int32), 2


def join_label(label2d, rank):
    if label2d is None:
        return None
    return label2d[:, :, None] if rank == 3 else label2d


def image_tensor(image):
    """[H, W, 3] float32 or uint8 as the kernels take it"""
    if image.dim() != 3 or image.shape[-1] != 3:
        raise ValueError(f"image must be [H, W, 3], got {tuple(image.shape)}")
    return image if image.dtype in (torch.float32, torch.uint8) else image.to(torch.float32)


def gather(image, label, out_size=None, offset=(0, 0), flip=False, rects=(), pad_value=(0.0, 0.0, 0.0), pad_label=255, photometric=None,
           seed=0):
    """image [H, W, 3], label as the sample has it -> (float32 [oh, ow, 3], label of the same rank).  photometric: {slot: value} of the float
    table (0 brightness delta, 1 contrast factor, 5 saturation factor, 6 hue delta, 7 evaluation-noise stddev)"""
    image = image_tensor(image)
    H, W = int(image.shape[0]), int(image.shape[1])
    oh, ow = (H, W) if out_size is None else (int(out_size[0]), int(out_size[1]))
    if len(rects) > MAX_RECTS:
        raise ValueError(f"one launch takes at most {MAX_RECTS} erase rectangles")
    lab2d, rank = split_label(label)
    tab = np.zeros((1, K.augment_params_ints()), dtype=np.int32)
    tab[0, :8] = [H, W, H, W, int(offset[0]), int(offset[1]), int(bool(flip)), len(rects)]
    for e, r in enumerate(rects):
        tab[0, 8 + 4 * e:12 + 4 * e] = r
    pdev = torch.from_numpy(tab).to(image.device)
    fdev = None
    if photometric:
        ftab = np.zeros((1, K.augment_params_floats()), dtype=np.float32)
        ftab[0, 1] = ftab[0, 5] = 1.0
        for slot, value in photometric.items():
            ftab[0, slot] = value
        fdev = torch.from_numpy(ftab).to(image.device)
        if ftab[0, 1] != 1.0:      # tf.image.adjust_contrast's reference point: the channel means, filled into slots 2..4 on the device
            K.augment_channel_means(image[None], pdev, fdev)
    out, out_lab = K.augment_crop_batch(image[None], None if lab2d is None else lab2d[None], pdev, [float(v) for v in pad_value],
                                        (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), int(pad_label), oh, ow, int(seed) & 0xFFFFFFFFFFFFFFFF, fparams=fdev)
    return out[0], join_label(None if out_lab is None else out_lab[0], rank)
