"""fp64 restatement of the reference's EfficientNet (backbones/efficientnet.py:117-372, build_dilated_efficientnet :492-507) on the oracle's
ops, addressed by the product's weight names.  It keeps the reference's literal form: a stride-2 block zero-pads by correct_pad and runs its
depthwise convolution with padding 'valid' (the product calls the strided 'same' operator), and the stem does the same -- so the padding
equivalence is tested, not assumed.  Test infrastructure only."""
import math

import torch

from oracle import models as OM
from oracle import tf_ops as O

BLOCKS = [(3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2), (5, 3, 80, 112, 6, 1), (5, 4, 112, 192, 6, 2),
          (3, 1, 192, 320, 6, 1)]      # kernel, repeats, filters_in, filters_out, expand_ratio, strides (se_ratio 0.25, id_skip everywhere)


def round_filters(filters, coefficient, divisor=8):
    filters *= coefficient
    new = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    if new < 0.9 * filters:
        new += divisor
    return int(new)


def plan(width=1.0, depth=1.0, output_stride=32):
    """per block: dict(name, k, filters_in, filters_out, expand, built_stride, stride, dilation, drop_index) after the dilation surgery"""
    out = []
    for i, (k, reps, fin, fout, exp, s) in enumerate(BLOCKS):
        fin, fout = round_filters(fin, width), round_filters(fout, width)
        for j in range(int(math.ceil(depth * reps))):
            out.append(dict(name=f"block{i + 1}{chr(j + 97)}_", k=k, filters_in=fin if j == 0 else fout, filters_out=fout, expand=exp,
                            built_stride=s if j == 0 else 1))
    current_os, dilation = 2, 1
    for b in out:
        if current_os >= output_stride:
            dilation *= b["built_stride"]
            b["stride"], b["dilation"] = 1, dilation
        else:
            current_os *= b["built_stride"]
            b["stride"], b["dilation"] = b["built_stride"], 1
    return out


def correct_pad(H, W, k):
    """imagenet_utils.correct_pad: ((top, bottom), (left, right))"""
    c = k // 2
    return (c - (1 - H % 2), c), (c - (1 - W % 2), c)


def _pad_valid(x, k):
    (t, b), (l, r) = correct_pad(x.shape[1], x.shape[2], k)
    return torch.nn.functional.pad(x, (0, 0, l, r, t, b))


def swish(t):
    return t * torch.sigmoid(t)


def se_tail(w, p, x):
    """reduce_mean -> se_reduce -> swish -> se_expand -> sigmoid -> multiply (:221-232)"""
    se = x.mean(dim=(1, 2), keepdim=True)
    se = swish(O.conv2d(se, w[f"{p}se_reduce/kernel"], w[f"{p}se_reduce/bias"], 1, 1, "same"))
    se = torch.sigmoid(O.conv2d(se, w[f"{p}se_expand/kernel"], w[f"{p}se_expand/bias"], 1, 1, "same"))
    return x * se


def efficientnet_forward(w, x, width=1.0, depth=1.0, output_stride=32, training=False, use_top=True, drop_factors=None, new_stats=None):
    """endpoint list of EfficientNet.call(return_endpoints=True) after build_dilated_efficientnet(output_stride); drop_factors: per-block
    per-sample drop-connect factors (None where a block has none)"""
    def bn(name, y):
        return OM._bn(w, name, y, training, 1e-3, new_stats=new_stats)

    x = swish(bn("stem_bn", O.conv2d(_pad_valid(x, 3), w["stem_conv/kernel"], None, 2, 1, "valid")))
    endpoints = []
    for i, b in enumerate(plan(width, depth, output_stride)):
        p = b["name"]
        if b["built_stride"] > 1:
            endpoints.append(x)
        inp = x
        if b["expand"] != 1:
            x = swish(bn(f"{p}expand_bn", O.conv2d(x, w[f"{p}expand_conv/kernel"], None, 1, 1, "same")))
        if b["stride"] == 2:
            x = O.depthwise_conv2d(_pad_valid(x, b["k"]), w[f"{p}dwconv/depthwise_kernel"], None, 2, 1, "valid")
        else:
            x = O.depthwise_conv2d(x, w[f"{p}dwconv/depthwise_kernel"], None, 1, b["dilation"], "same")
        x = se_tail(w, p, swish(bn(f"{p}bn", x)))
        x = bn(f"{p}project_bn", O.conv2d(x, w[f"{p}project_conv/kernel"], None, 1, 1, "same"))
        if b["stride"] == 1 and b["filters_in"] == b["filters_out"]:
            f = drop_factors[i] if drop_factors is not None else None
            if training and f is not None:
                x = x * f.reshape(-1, 1, 1, 1)
            x = x + inp
    if use_top:
        x = swish(bn("top_bn", O.conv2d(x, w["top_conv/kernel"], None, 1, 1, "same")))
    return endpoints + [x]


def efficientnet_aspp_forward(w, x, training=False, output_stride=32, drop_factors=None, head="aspp_head", seg="seg", new_stats=None):
    """heads.efficientnet_b0_aspp: B0 -> ASPP -> end_conv -> logits_conv -> bilinear resize (the composition of OM.convnext_aspp_forward)"""
    ends = efficientnet_forward(w, x, output_stride=output_stride, training=training, drop_factors=drop_factors, new_stats=new_stats)
    mult = max(32 // output_stride, 1)
    feat = OM.aspp(w, f"{head}/aspp", ends[-1], training, rates=tuple(r * mult for r in (3, 6, 9)), new_stats=new_stats)
    feat = OM.conv_norm_act(w, f"{head}/end_conv", feat, training, new_stats=new_stats)
    small = O.conv2d(feat, w[f"{seg}/logits_conv/kernel"], w[f"{seg}/logits_conv/bias"], 1, 1, "same")
    return {"endpoints": ends, "logits": O.resize_bilinear(small, (x.shape[1], x.shape[2]))}
