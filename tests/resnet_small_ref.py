"""fp64 restatement of the reference's ResNet-9 / 10 / 18 (backbones/resnet_common.py:348-418 constructors, :24-184 Stack / Stack2, :187-345
ResNet with the 3x3 stem, :561-598 build_atrous_resnet / apply_multi_grid; backbones/resnet_blocks_small.py BlockType2Small) on the oracle's
ops, addressed by the product's weight names: the block table, the stride / dilation surgery, the basic block and the endpoint rule.  Test
infrastructure only."""
import torch

from oracle import models as OM
from oracle import tf_ops as O

EPS = 1.001e-5
FILTERS = [64, 128, 256, 512]
BLOCKS = {"resnet9": [1, 1, 1, 1], "resnet10": [1, 1, 1, 1], "resnet18": [2, 2, 2, 2]}


def stem_widths(name):
    """conv1_1 / conv1_2 / conv1_3 widths of the 3x3 stem: int(64 m0), int(64 m1), int(128 m2)"""
    m = (0.375, 0.5, 0.5) if name == "resnet10" else (0.5, 0.5, 0.5)
    return [int(64 * m[0]), int(64 * m[1]), int(128 * m[2])]


def plan(name, output_stride=32, slim=True, multi_grids=(1, 2, 4)):
    """per stack, per block: dict(name, filters, cin, built_stride, conv_shortcut (after build()'s width rule), stride, rate) after
    build_atrous_resnet(output_stride) and apply_multi_grid(block_index=-1)"""
    counts = BLOCKS[name]
    stack_strides = [2, 2, 2, 1] if slim else [1, 2, 2, 2]
    cin = stem_widths(name)[-1]
    stacks = []
    for si, (f, nb, s1) in enumerate(zip(FILTERS, counts, stack_strides)):
        if slim:      # Stack2: the stride on the last block, the shortcut conv on the first
            spec = [(s1, True)] if nb == 1 else [(1, True)] + [(1, False)] * (nb - 2) + [(s1, False)]
        else:         # Stack: both on the first block
            spec = [(s1, True)] + [(1, False)] * (nb - 1)
        blocks = []
        for bi, (s, cs) in enumerate(spec):
            blocks.append(dict(name=f"conv{si + 2}_block{bi + 1}", filters=f, cin=cin, built_stride=s, conv_shortcut=cs and cin != f,
                               stride=s, rate=1))
            cin = f
        stacks.append(dict(blocks=blocks, endpoint=s1 > 1, slim=slim))
    current_os, rate = 4, 1
    for st in stacks:
        for b in st["blocks"]:
            if b["stride"] > 1:
                if current_os >= output_stride:
                    rate *= 2
                    b["stride"] = 1
                    b["rate"] = b["rate"] * rate
                else:
                    current_os *= 2
            else:
                b["rate"] = b["rate"] * rate
    for i, b in enumerate(stacks[-1]["blocks"]):
        b["rate"] = b["rate"] * multi_grids[i]
    return stacks


def weight_names(name, slim=True):
    """trainable weights (kernels, BN gamma / beta, no biases) in the reference's names"""
    names = []
    for i in (1, 2, 3):
        names += [f"conv1_{i}_conv/kernel", f"conv1_{i}_bn/gamma", f"conv1_{i}_bn/beta"]
    for st in plan(name, slim=slim):
        for b in st["blocks"]:
            ks = ("0", "1", "2") if b["conv_shortcut"] else ("1", "2")
            for k in ks:
                names += [f"{b['name']}_{k}_conv/kernel", f"{b['name']}_{k}_bn/gamma", f"{b['name']}_{k}_bn/beta"]
    return names


def parameter_count(name, slim=True):
    """from the block table: convolution kernels plus BN gamma / beta"""
    widths = stem_widths(name)
    n, cin = 0, 3
    for w in widths:
        n += 9 * cin * w + 2 * w
        cin = w
    for st in plan(name, slim=slim):
        for b in st["blocks"]:
            f = b["filters"]
            n += 9 * b["cin"] * f + 2 * f + 9 * f * f + 2 * f
            if b["conv_shortcut"]:
                n += b["cin"] * f + 2 * f
    return n


def tail_pre(w, name, z2, sc, stride, conv_shortcut, training, new_stats=None):
    """bn2(z2) + avg_pool_s(bn0(z0) or x), the tail before its ReLU -- BlockType2Small.call :88-107 after the convolutions"""
    if conv_shortcut:
        sc = OM._bn(w, f"{name}_0_bn", sc, training, EPS, new_stats=new_stats)
    if stride > 1:
        sc = O.avg_pool_same(sc, stride, stride)
    return sc + OM._bn(w, f"{name}_2_bn", z2, training, EPS, new_stats=new_stats)


def tail(w, name, z2, sc, stride, conv_shortcut, training, new_stats=None):
    """relu(bn2(z2) + avg_pool_s(bn0(z0) or x)) (:108)"""
    return torch.relu(tail_pre(w, name, z2, sc, stride, conv_shortcut, training, new_stats))


def block(w, b, x, training, new_stats=None):
    """BlockType2Small.call (:84-119)"""
    name = b["name"]
    sc = O.conv2d(x, w[f"{name}_0_conv/kernel"], None, 1, 1, "same") if b["conv_shortcut"] else x
    y = O.conv2d(x, w[f"{name}_1_conv/kernel"], None, b["stride"], b["rate"], "same")
    y = torch.relu(OM._bn(w, f"{name}_1_bn", y, training, EPS, new_stats=new_stats))
    z2 = O.conv2d(y, w[f"{name}_2_conv/kernel"], None, 1, b["rate"], "same")
    return tail(w, name, z2, sc, b["stride"], b["conv_shortcut"], training, new_stats)


def resnet_forward(w, x, name="resnet18", output_stride=32, slim=True, training=False, new_stats=None):
    """endpoint list of ResNet.call(return_endpoints=True) with the 3x3 stem after the atrous surgery"""
    for i, s in ((1, 2), (2, 1), (3, 1)):
        x = torch.relu(OM._bn(w, f"conv1_{i}_bn", O.conv2d(x, w[f"conv1_{i}_conv/kernel"], None, s, 1, "same"), training, EPS,
                              new_stats=new_stats))
    endpoints = [x]
    x = O.max_pool_same(x, 3, 1 if output_stride == 2 else 2)
    for st in plan(name, output_stride, slim):
        blocks = st["blocks"]
        for bi, b in enumerate(blocks):
            if st["endpoint"] and bi == (len(blocks) - 1 if slim else 0):
                endpoints.append(x)      # the value before the stack's (possibly removed) stride
            x = block(w, b, x, training, new_stats)
    endpoints.append(x)
    return endpoints


def resnet_aspp_forward(w, x, name="resnet18", training=False, output_stride=32, head="aspp_head", seg="seg", new_stats=None):
    """heads.resnet18_aspp: ResNet-18 -> ASPP -> end_conv -> logits_conv -> bilinear resize"""
    ends = resnet_forward(w, x, name=name, output_stride=output_stride, training=training, new_stats=new_stats)
    mult = max(32 // output_stride, 1)
    feat = OM.aspp(w, f"{head}/aspp", ends[-1], training, rates=tuple(r * mult for r in (3, 6, 9)), new_stats=new_stats)
    feat = OM.conv_norm_act(w, f"{head}/end_conv", feat, training, new_stats=new_stats)
    small = O.conv2d(feat, w[f"{seg}/logits_conv/kernel"], w[f"{seg}/logits_conv/bias"], 1, 1, "same")
    return {"endpoints": ends, "logits": O.resize_bilinear(small, (x.shape[1], x.shape[2]))}
