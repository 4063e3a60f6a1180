"""backbones/resnet_blocks_small.py of the reference: BlockType2Small (:10-119), the basic block of ResNet-9 / 10 / 18 -- two 3x3
convolutions, stride and dilation on the first, an un-strided 1x1 shortcut convolution that build() drops when the input width already equals
`filters`, and a SAME average pool of the shortcut by the live stride.  BN epsilon 1.001e-5."""
from .. import functional as F
from .. import nn
from ..layers.base_layers import Conv2D
from ..layers.normalizations import normalization
from ..nn import Layer
from .resnet_blocks import BN_EPSILON, _bn_relu, _pair

DEFAULT_CONV_FUNC = Conv2D


class BlockType2Small(Layer):
    def __init__(self, filters, kernel_size=3, stride=1, conv_shortcut=True, use_bias=False, norm_method=None, downsample_method="avg",
                 conv_func=DEFAULT_CONV_FUNC, name=None):
        super().__init__(name=name)
        self.filters = filters
        self.conv_shortcut = conv_shortcut
        self.downsample_method = downsample_method
        self.use_bias = use_bias
        self.norm_method = norm_method
        self.conv_func = conv_func
        self.conv1_conv = conv_func(filters, kernel_size, strides=stride, padding="SAME", use_bias=use_bias, name=name + "_1_conv")
        self.conv1_bn = normalization(epsilon=BN_EPSILON, method=norm_method, name=name + "_1_bn")
        self.conv2_conv = conv_func(filters, kernel_size, padding="SAME", use_bias=use_bias, name=name + "_2_conv")
        self.conv2_bn = normalization(epsilon=BN_EPSILON, method=norm_method, name=name + "_2_bn")

    def build(self, input_shape):      # (:44-58)
        if input_shape[-1] == self.filters:
            self.conv_shortcut = False
        if self.conv_shortcut:
            self.shortcut_conv = self.conv_func(self.filters, kernel_size=1, use_bias=self.use_bias, name=self.name + "_0_conv")
            self.shortcut_bn = normalization(epsilon=BN_EPSILON, method=self.norm_method, name=self.name + "_0_bn")
        self.built = True

    @property
    def strides(self):
        return self.conv1_conv.strides[0]

    @strides.setter
    def strides(self, value):
        self.conv1_conv.strides = _pair(value)

    @property
    def atrous_rates(self):
        return self.conv1_conv.dilation_rate[0]

    @atrous_rates.setter
    def atrous_rates(self, value):
        value = _pair(value)
        self.conv1_conv.dilation_rate = value
        self.conv2_conv.dilation_rate = value

    def _tail_fusable(self):
        """both norms BatchNormalization, an average-pooled shortcut, and not a shape-only (dry) run"""
        norms = (self.conv2_bn, self.shortcut_bn) if self.conv_shortcut else (self.conv2_bn,)
        return (not nn.dry_run() and F.resblock_fused_enabled() and all(hasattr(n, "moving_mean") for n in norms)
                and (self.strides == 1 or "avg" in self.downsample_method))

    def call(self, inputs, training=None, **kwargs):      # (:84-119)
        inputs, shortcut = F.fork(inputs, 2)      # two consumers: their gradients are summed by our own kernel, not by the engine's add
        st = _pair(self.conv1_conv.strides)
        if self.conv_shortcut:
            shortcut = self.shortcut_conv(shortcut)
        if self._tail_fusable():
            x = _bn_relu(self.conv1_bn, self.conv1_conv(inputs), training)
            z2 = self.conv2_conv(x)
            return F.resblock_tail(z2, self.conv2_bn, shortcut, self.shortcut_bn if self.conv_shortcut else None, st, training)
        if self.conv_shortcut:
            shortcut = self.shortcut_bn(shortcut, training=training)
        if self.strides > 1:
            if "avg" in self.downsample_method:
                shortcut = F.avg_pool2d(shortcut, st, st, "same")
            elif "max" in self.downsample_method:
                shortcut = F.max_pool2d(shortcut, st, st, "same")
            else:
                raise ValueError("Only max or avg are supported")
        x = _bn_relu(self.conv1_bn, self.conv1_conv(inputs), training)
        x = self.conv2_bn(self.conv2_conv(x), training=training)
        return F.add_relu(shortcut, x)
