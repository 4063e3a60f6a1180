"""fp64 restatement of the reference's JointPyramidUpsampling (layers/jpu.py:19-90) on the oracle's ops, addressed by the product's weight names:
three 3x3 ConvNormAct on the last three endpoints, bilinear resize to the first one's size, concat, then per dilation 1 / 2 / 4 / 8 a depthwise 3x3
WITH bias -> BN -> 1x1 ConvNormAct, concat.  Also the composed tail alone (what functional.jpu_tail computes) and a loop-based numpy depthwise
convolution that the restatement is checked against.  Test infrastructure only."""
import numpy as np
import torch

from oracle import models as OM
from oracle import tf_ops as O

RATES = (1, 2, 4, 8)


def weight_names(name="jpu"):
    """trainable weights in the reference's names"""
    names = []
    for i in range(3):
        names += [f"{name}/endpoint_conv_{i}/conv/kernel", f"{name}/endpoint_conv_{i}/bn/gamma", f"{name}/endpoint_conv_{i}/bn/beta"]
    for r in RATES:
        names += [f"{name}/end_depthwise_conv_{r}/depthwise_kernel", f"{name}/end_depthwise_conv_{r}/bias"]
        names += [f"{name}/end_depthwise_bn_{r}/gamma", f"{name}/end_depthwise_bn_{r}/beta"]
        names += [f"{name}/end_pointwise_convs_{r}/conv/kernel", f"{name}/end_pointwise_convs_{r}/bn/gamma", f"{name}/end_pointwise_convs_{r}/bn/beta"]
    return names


def branch_pre(w, name, r, merged, training, new_stats=None):
    """one branch up to the pointwise convolution's output (:82-84 without the pointwise block's BN and ReLU)"""
    x = O.depthwise_conv2d(merged, w[f"{name}/end_depthwise_conv_{r}/depthwise_kernel"], w[f"{name}/end_depthwise_conv_{r}/bias"], 1, r, "same")
    x = OM._bn(w, f"{name}/end_depthwise_bn_{r}", x, training, 1e-3, new_stats=new_stats)
    return O.conv2d(x, w[f"{name}/end_pointwise_convs_{r}/conv/kernel"], None, 1, 1, "same")


def jpu_forward(w, endpoints, name="jpu", training=False, new_stats=None):
    """JointPyramidUpsampling.call (:61-90)"""
    assert len(endpoints) >= 3
    endpoints = list(endpoints)[-3:]
    size = endpoints[0].shape[1:3]
    for i in range(3):
        e = OM.conv_norm_act(w, f"{name}/endpoint_conv_{i}", endpoints[i], training, new_stats=new_stats)
        endpoints[i] = O.resize_bilinear(e, size)
    merged = torch.cat(endpoints, dim=-1)
    results = []
    for r in RATES:
        p = f"{name}/end_pointwise_convs_{r}"
        x = branch_pre(w, name, r, merged, training, new_stats)
        results.append(torch.relu(OM._bn(w, f"{p}/bn", x, training, 1e-3, new_stats=new_stats)))
    return torch.cat(results, dim=-1)


def resnet18_jpu_aspp_forward(w, x, training=False, head="jpu_aspp_head", seg="seg", new_stats=None):
    """heads.resnet18_jpu_aspp: ResNet-18 (stride 32) -> JPU -> ASPP (rates x 4) -> end_conv -> logits_conv -> bilinear resize"""
    from tests import resnet_small_ref as R

    ends = R.resnet_forward(w, x, name="resnet18", output_stride=32, training=training, new_stats=new_stats)
    feat = jpu_forward(w, ends, f"{head}/jpu", training, new_stats)
    feat = OM.aspp(w, f"{head}/aspp", feat, training, rates=(12, 24, 36), new_stats=new_stats)
    feat = OM.conv_norm_act(w, f"{head}/end_conv", feat, training, new_stats=new_stats)
    small = O.conv2d(feat, w[f"{seg}/logits_conv/kernel"], w[f"{seg}/logits_conv/bias"], 1, 1, "same")
    return {"endpoints": ends, "logits": O.resize_bilinear(small, (x.shape[1], x.shape[2]))}


def depthwise_loops(x, kernel, bias, rate):
    """DepthwiseConv2D(3, padding="same", dilation_rate=rate) with loops over numpy arrays: x [N, H, W, C], kernel [3, 3, C, 1], bias [C].
    'same' at stride 1: the output has the input's size, tap (i, j) reads (h + (i - 1) rate, w + (j - 1) rate), zero outside the image."""
    N, H, W, C = x.shape
    out = np.zeros((N, H, W, C), dtype=np.float64)
    for n in range(N):
        for h in range(H):
            for ww in range(W):
                acc = np.array(bias, dtype=np.float64).copy()
                for i in range(3):
                    for j in range(3):
                        hh, wq = h + (i - 1) * rate, ww + (j - 1) * rate
                        if 0 <= hh < H and 0 <= wq < W:
                            acc += x[n, hh, wq, :] * kernel[i, j, :, 0]
                out[n, h, ww, :] = acc
    return out
