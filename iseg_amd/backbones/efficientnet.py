"""EfficientNet B0-B7 / L2 (backbones/efficientnet.py of the reference): DEFAULT_BLOCKS_ARGS :22-92, round_filters / round_repeats :101-114,
Block :117-255, EfficientNet :258-372, EfficientNetB0 ... L2 :375-489, build_dilated_efficientnet :492-507 -- same classes, attributes
(`blocks`, `dwconv.strides` / `.dilation_rate` the dilation surgery edits, `output_endpoint`) and weight names (stem_conv, stem_bn,
block{i}{a..}_{expand_conv, expand_bn, dwconv, bn, se_reduce, se_expand, project_conv, project_bn}, top_conv, top_bn), so a Keras .h5
converted to .npz loads by name.

A stride-2 block of the reference zero-pads by correct_pad and runs its k x k depthwise convolution with padding "valid"; for k = 3 and
k = 5 that is exactly TF's 'same' sampling at stride 2 (even sizes pad (k//2 - 1, k//2), odd ones (k//2, k//2)), so the block calls the
strided 'same' depthwise operator (functional.depthwise_conv2d(strides=2)) and no padded copy of the activation exists.  The stem's
correct_pad + 3 x 3 / s2 'valid' convolution is the 'same' stride-2 convolution for the same reason.

The tail of every block -- dwconv_bn -> swish -> squeeze-excite -> gate -- runs as one fused operator (functional.bn_swish_se,
csrc/mbconv.hip) that never writes the un-gated activation.  ISEG_MBCONV_FUSED=0 selects the composition of the existing kernels
(batch_norm, swish, global_avg_pool, two 1 x 1 convolutions, sigmoid, channel gate): the A/B baseline, and the route of any shape the fused
kernels refuse."""
import copy
import math

from .. import functional as F
from .. import nn as _nn
from ..layers.base_layers import Conv2D, DepthwiseConv2D
from ..layers.nasfpn import _ChannelGateFn, _SigmoidGateFn
from ..layers.normalizations import normalization
from ..nn import Layer

DEFAULT_BLOCKS_ARGS = [
    {"kernel_size": 3, "repeats": 1, "filters_in": 32, "filters_out": 16, "expand_ratio": 1, "id_skip": True, "strides": 1, "se_ratio": 0.25},
    {"kernel_size": 3, "repeats": 2, "filters_in": 16, "filters_out": 24, "expand_ratio": 6, "id_skip": True, "strides": 2, "se_ratio": 0.25},
    {"kernel_size": 5, "repeats": 2, "filters_in": 24, "filters_out": 40, "expand_ratio": 6, "id_skip": True, "strides": 2, "se_ratio": 0.25},
    {"kernel_size": 3, "repeats": 3, "filters_in": 40, "filters_out": 80, "expand_ratio": 6, "id_skip": True, "strides": 2, "se_ratio": 0.25},
    {"kernel_size": 5, "repeats": 3, "filters_in": 80, "filters_out": 112, "expand_ratio": 6, "id_skip": True, "strides": 1, "se_ratio": 0.25},
    {"kernel_size": 5, "repeats": 4, "filters_in": 112, "filters_out": 192, "expand_ratio": 6, "id_skip": True, "strides": 2, "se_ratio": 0.25},
    {"kernel_size": 3, "repeats": 1, "filters_in": 192, "filters_out": 320, "expand_ratio": 6, "id_skip": True, "strides": 1, "se_ratio": 0.25},
]

CONV_KERNEL_INITIALIZER = "he_truncated_normal_fan_out"      # VarianceScaling(2.0, "fan_out", "truncated_normal")


def round_filters(filters, coefficient, divisor=8):
    """Round number of filters based on depth multiplier."""
    filters *= coefficient
    new_filters = max(divisor, int(filters + divisor / 2) // divisor * divisor)
    if new_filters < 0.9 * filters:      # rounding down must not lose more than 10 %
        new_filters += divisor
    return int(new_filters)


def round_repeats(repeats, depth_coefficient):
    """Round number of repeats based on depth multiplier."""
    return int(math.ceil(depth_coefficient * repeats))


class Block(Layer):
    def __init__(self, activation=None, drop_rate=0, filters_in=32, filters_out=16, kernel_size=3, strides=1, expand_ratio=1, se_ratio=0,
                 id_skip=True, name=None, **kwargs):
        super().__init__(name=name)
        self.strides = strides
        self.kernel_size = kernel_size
        self.activation = activation if activation is not None else F.swish
        self.filters_in = filters_in
        self.filters_out = filters_out
        self.drop_rate = drop_rate
        self.id_skip = id_skip
        self.output_endpoint = strides > 1
        self.drop_path_mask = None      # per-sample drop-connect factors injected by parity tests (F.drop_path's `mask`)
        self.filters = filters = filters_in * expand_ratio
        if expand_ratio != 1:
            self.expand_conv = Conv2D(filters, 1, padding="same", use_bias=False, kernel_initializer=CONV_KERNEL_INITIALIZER, name=name + "expand_conv")
            self.expand_conv_bn = normalization(name=name + "expand_bn")
        else:
            self.expand_conv = self.expand_conv_bn = None
        self.dwconv = DepthwiseConv2D(kernel_size, strides=strides, padding="same", use_bias=False, depthwise_initializer=CONV_KERNEL_INITIALIZER,
                                      name=name + "dwconv")
        self.dwconv_bn = normalization(name=name + "bn")
        if 0 < se_ratio <= 1:
            self.filters_se = max(1, int(filters_in * se_ratio))
            self.se_reduce = Conv2D(self.filters_se, 1, padding="same", kernel_initializer=CONV_KERNEL_INITIALIZER, name=name + "se_reduce")
            self.se_expand = Conv2D(filters, 1, padding="same", kernel_initializer=CONV_KERNEL_INITIALIZER, name=name + "se_expand")
        else:
            self.se_reduce = self.se_expand = None
        self.project_conv = Conv2D(filters_out, 1, padding="same", use_bias=False, kernel_initializer=CONV_KERNEL_INITIALIZER,
                                   name=name + "project_conv")
        self.project_bn = normalization(name=name + "project_bn")

    def build(self, input_shape):
        # the fused tail reads these layers' weights without calling them: build them from the known widths
        for layer, cin in ((self.dwconv_bn, self.filters), (self.se_reduce, self.filters), (self.se_expand, getattr(self, "filters_se", 0))):
            if layer is not None and not layer.built:
                layer.build((1, 1, 1, cin))
                layer.built = True
        self.built = True

    def _bn_swish_se(self, x, training):
        bn = self.dwconv_bn
        bn_training = bool(training) and bn.trainable
        if self.se_reduce is None:
            return self.activation(bn(x, training=training))
        if self.activation is F.swish and F.mbconv_fused_enabled() and (
                _nn.dry_run() or F.bn_swish_se_supported(x, self.filters_se, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance)):
            return F.bn_swish_se(x, bn.gamma, bn.beta, bn.moving_mean, bn.moving_variance, bn.epsilon, bn.momentum, bn_training,
                                 self.se_reduce.kernel, self.se_reduce.bias, self.se_expand.kernel, self.se_expand.bias, sync=bn.synchronized)
        x = self.activation(bn(x, training=training))
        x, gated = F.fork(x, 2)
        se = self.activation(self.se_reduce(F.global_avg_pool(x)))
        se = self.se_expand(se)
        if _nn.dry_run():
            return gated
        return _ChannelGateFn.apply(gated, _SigmoidGateFn.apply(se))

    def call(self, inputs, training=None):
        current_strides = self.dwconv.strides[0]
        residual = self.id_skip and current_strides == 1 and self.filters_in == self.filters_out
        x, skip = F.fork(inputs, 2) if residual else (inputs, None)
        if self.expand_conv is not None:
            x = self.activation(self.expand_conv_bn(self.expand_conv(x), training=training))
        x = self._bn_swish_se(self.dwconv(x), training)
        x = self.project_bn(self.project_conv(x), training=training)
        if residual:
            if self.drop_rate > 0:      # Dropout(drop_rate, noise_shape=(None, 1, 1, 1)): one factor per sample
                x = F.drop_path(x, self.drop_rate, bool(training), mask=self.drop_path_mask)
            x = F.add(skip, x)
        return x


class EfficientNet(Layer):
    def __init__(self, width_confficient, depth_confficient, drop_connect_rate=0.2, depth_divisor=8, activation=None, blocks_args="default",
                 use_top=True, return_endpoints=False, name="efficientnet", **kwargs):
        super().__init__(name=name)
        import torch

        self.use_top = use_top
        self.return_endpoints = return_endpoints
        if blocks_args == "default":
            blocks_args = DEFAULT_BLOCKS_ARGS
        blocks_args = copy.deepcopy(blocks_args)
        self.activation = activation if activation is not None else F.swish
        self.stem_conv = Conv2D(round_filters(32, width_confficient, depth_divisor), 3, strides=2, padding="same", use_bias=False,
                                kernel_initializer=CONV_KERNEL_INITIALIZER, name="stem_conv")
        self.steam_conv_bn = normalization(name="stem_bn")      # (sic) attribute name of the reference
        self.blocks = torch.nn.ModuleList()
        b = 0
        blocks_num = float(sum(round_repeats(args["repeats"], depth_confficient) for args in blocks_args))
        for i, args in enumerate(blocks_args):
            assert args["repeats"] > 0
            args["filters_in"] = round_filters(args["filters_in"], width_confficient, depth_divisor)
            args["filters_out"] = round_filters(args["filters_out"], width_confficient, depth_divisor)
            for j in range(round_repeats(args.pop("repeats"), depth_confficient)):
                if j > 0:
                    args["strides"] = 1
                    args["filters_in"] = args["filters_out"]
                self.blocks.append(Block(activation=self.activation, drop_rate=drop_connect_rate * b / blocks_num,
                                         name="block{}{}_".format(i + 1, chr(j + 97)), **args))
                b += 1
        if use_top:
            self.top_conv = Conv2D(round_filters(1280, width_confficient, depth_divisor), 1, padding="same", use_bias=False,
                                   kernel_initializer=CONV_KERNEL_INITIALIZER, name="top_conv")
            self.top_bn = normalization(name="top_bn")

    def call(self, inputs, training=None, **kwargs):
        endpoints = []
        x = self.activation(self.steam_conv_bn(self.stem_conv(F.cast_input(inputs)), training=training))
        for block in self.blocks:
            if block.output_endpoint:
                if self.return_endpoints:
                    x, e = F.fork(x, 2)
                    endpoints.append(e)
            x = block(x, training=training)
        if self.use_top:
            x = self.activation(self.top_bn(self.top_conv(x), training=training))
        endpoints.append(x)
        return endpoints if self.return_endpoints else x


def _efficientnet(width, depth, drop_connect_rate, name):
    def make(return_endpoints=False, use_top=True, default_size=None):      # default_size is accepted and dropped, as the reference does
        return EfficientNet(width_confficient=width, depth_confficient=depth, drop_connect_rate=drop_connect_rate, use_top=use_top,
                            return_endpoints=return_endpoints, name=name)

    make.__name__ = name
    return make


EfficientNetB0 = _efficientnet(1.0, 1.0, 0.2, "efficientnetb0")
EfficientNetB1 = _efficientnet(1.0, 1.1, 0.2, "efficientnetb1")
EfficientNetB2 = _efficientnet(1.1, 1.2, 0.3, "efficientnetb2")
EfficientNetB3 = _efficientnet(1.2, 1.4, 0.3, "efficientnetb3")
EfficientNetB4 = _efficientnet(1.4, 1.8, 0.4, "efficientnetb4")
EfficientNetB5 = _efficientnet(1.6, 2.2, 0.4, "efficientnetb5")
EfficientNetB6 = _efficientnet(1.8, 2.6, 0.5, "efficientnetb6")
EfficientNetB7 = _efficientnet(2.0, 3.1, 0.5, "efficientnetb7")
EfficientNetL2 = _efficientnet(4.3, 5.3, 0.5, "efficientnetl2")


def build_dilated_efficientnet(efficientnet, output_stride=16):
    """from output stride 2 on, tested BEFORE a block's own stride is applied: every block once the stride is reached runs at stride 1,
    padding 'same' and the running dilation (endpoints stay where the blocks were built with strides > 1)"""
    current_os = 2
    current_dilation = 1
    for block in efficientnet.blocks:
        if current_os >= output_stride:
            current_dilation *= block.dwconv.strides[0]
            block.dwconv.strides = (1, 1)
            block.dwconv.padding = "same"
            block.dwconv.dilation_rate = (current_dilation, current_dilation)
        else:
            current_os *= block.dwconv.strides[0]
    return efficientnet
