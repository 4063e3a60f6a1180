"""fp64 restatement of the reference's Xception-65 (backbones/xception_common.py:14-258) on the oracle's ops, addressed by the product's weight
names: the block table, build_atrous_xception, the two kinds of separable unit, the shortcut kinds and the endpoint rule.  Test infrastructure
only."""
import torch

from oracle import models as OM
from oracle import tf_ops as O

# filters_list, built stride, skip_connection, activation, repeat (xception65 :227-238)
BLOCKS = [([128, 128, 128], 2, 2, False, 1), ([256, 256, 256], 2, 2, False, 1), ([728, 728, 728], 2, 2, False, 1),
          ([728, 728, 728], 1, 1, False, 16), ([728, 1024, 1024], 2, 2, False, 1), ([1536, 1536, 2048], 1, 0, True, 1)]


def plan(output_stride=32):
    """per block: dict(index, filters, skip, activation, built_stride, stride, rate) after build_atrous_xception"""
    out = []
    for filters, s, skip, act, rep in BLOCKS:
        for _ in range(rep):
            out.append(dict(index=len(out) + 2, filters=list(filters), skip=skip, activation=act, built_stride=s))
    current_os, rate = 2, 1
    for b in out:
        b["stride"], b["rate"] = b["built_stride"], 1
        if current_os >= output_stride:
            b["rate"] = rate
            rate *= b["stride"]
            b["stride"] = 1
        else:
            current_os *= b["stride"]
    return out


def weight_names():
    """trainable weights (kernels, BN gamma / beta) in the reference's names"""
    names = ["block1_conv1/kernel", "block1_conv2/kernel"] + [f"block1_conv{i}_BN/{v}" for i in (1, 2) for v in ("gamma", "beta")]
    for b in plan():
        for j in range(1, 4):
            p = f"block{b['index']}_separable_conv{j}"
            names += [f"{p}_depthwise/depthwise_kernel", f"{p}_pointwise/kernel"]
            names += [f"{p}_{k}_BN/{v}" for k in ("depthwise", "pointwise") for v in ("gamma", "beta")]
        if b["skip"] == 2:
            names += [f"block{b['index']}_shortcut/kernel", f"block{b['index']}_shortcut_BN/gamma", f"block{b['index']}_shortcut_BN/beta"]
    return names


def parameter_count():
    """from the block table: convolution kernels plus BN gamma / beta"""
    n = 3 * 3 * 3 * 32 + 2 * 32 + 3 * 3 * 32 * 64 + 2 * 64
    cin = 64
    for b in plan():
        c = cin
        for f in b["filters"]:
            n += 9 * c + 2 * c + c * f + 2 * f
            c = f
        if b["skip"] == 2:
            n += cin * b["filters"][-1] + 2 * b["filters"][-1]
        cin = b["filters"][-1]
    return n


def separable_unit(w, p, x, stride, rate, activation, training, new_stats=None):
    """XceptionDepthWiseConv.call (:47-62)"""
    def bn(name, y):
        return OM._bn(w, name, y, training, 1e-3, new_stats=new_stats)

    if not activation:
        x = torch.relu(x)
    x = O.depthwise_conv2d(x, w[f"{p}_depthwise/depthwise_kernel"], None, stride, rate, "same")
    x = bn(f"{p}_depthwise_BN", x)
    if activation:
        x = torch.relu(x)
    x = bn(f"{p}_pointwise_BN", O.conv2d(x, w[f"{p}_pointwise/kernel"], None, 1, 1, "same"))
    if activation:
        x = torch.relu(x)
    return x


def xception_forward(w, x, output_stride=32, training=False, new_stats=None):
    """endpoint list of Xception.call(return_endpoints=True) after build_atrous_xception(output_stride)"""
    def bn(name, y):
        return OM._bn(w, name, y, training, 1e-3, new_stats=new_stats)

    x = torch.relu(bn("block1_conv1_BN", O.conv2d(x, w["block1_conv1/kernel"], None, 2, 1, "same")))
    endpoints = [x]
    x = torch.relu(bn("block1_conv2_BN", O.conv2d(x, w["block1_conv2/kernel"], None, 1, 1, "same")))
    for b in plan(output_stride):
        if b["stride"] > 1:
            endpoints.append(x)
        inp = x
        n = len(b["filters"])
        for j in range(n):
            s = b["stride"] if j == n - 1 else 1
            x = separable_unit(w, f"block{b['index']}_separable_conv{j + 1}", x, s, b["rate"], b["activation"], training, new_stats)
        if b["skip"] == 1:
            x = x + inp
        elif b["skip"] == 2:
            p = f"block{b['index']}_shortcut"
            x = x + bn(f"{p}_BN", O.conv2d(inp, w[f"{p}/kernel"], None, b["stride"], 1, "same"))
    return endpoints + [x]


def xception_aspp_forward(w, x, training=False, output_stride=16, head="aspp_head", seg="seg", new_stats=None):
    """heads.xception65_aspp: Xception-65 -> ASPP -> end_conv -> logits_conv -> bilinear resize"""
    ends = xception_forward(w, x, output_stride=output_stride, training=training, new_stats=new_stats)
    mult = max(32 // output_stride, 1)
    feat = OM.aspp(w, f"{head}/aspp", ends[-1], training, rates=tuple(r * mult for r in (3, 6, 9)), new_stats=new_stats)
    feat = OM.conv_norm_act(w, f"{head}/end_conv", feat, training, new_stats=new_stats)
    small = O.conv2d(feat, w[f"{seg}/logits_conv/kernel"], w[f"{seg}/logits_conv/bias"], 1, 1, "same")
    return {"endpoints": ends, "logits": O.resize_bilinear(small, (x.shape[1], x.shape[2]))}
