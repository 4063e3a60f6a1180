"""Xception-65 (backbones/xception_common.py of the reference): XceptionDepthWiseConv :14-78, XceptionBlock :81-160, Xception :163-224,
xception65 :227-238, build_atrous_xception :241-258 -- same classes, attributes (`strides` / `atrous_rates` properties the atrous surgery
edits, `xception_blocks`) and weight names (block1_conv{1,2}[_BN], block{i}_separable_conv{j}_{depthwise,pointwise}[_BN],
block{i}_shortcut[_BN]), so a Keras .h5 converted to .npz loads by name.

The `activation=False` unit -- relu -> depthwise 3 x 3 -> BN -> pointwise 1 x 1 -- is 60 of the network's 63 units.  It runs as one operator
(functional.sepconv_unit, csrc/sepconv.hip): relu(x) is never written, the depthwise BN is folded into the pointwise GEMM's weights and bias,
and the backward forms the depthwise output gradient in LDS.  ISEG_SEPCONV_FUSED=0 selects the composition of the existing operators (relu,
depthwise_conv2d, batch_norm, conv2d): the A/B baseline, and the route of any shape or tensor the fused kernels refuse."""
from .. import functional as F
from ..layers.base_layers import Conv2D, DepthwiseConv2D
from ..layers.normalizations import normalization
from ..nn import Layer


def _pair(value):
    return tuple(int(v) for v in value) if isinstance(value, (tuple, list)) else (int(value), int(value))


class XceptionDepthWiseConv(Layer):
    def __init__(self, block_index, conv_index, filters, strides=(1, 1), activation=False, weight_decay=0.0, momentun=0.9):
        prefix = "block" + str(block_index) + "_separable_conv" + str(conv_index)
        super().__init__(name=prefix)
        self.activation = activation
        self.filters = int(filters)
        self.depthwise_conv = DepthwiseConv2D((3, 3), strides=strides, padding="same", use_bias=False, name=prefix + "_depthwise")
        self.depthwise_bn = normalization(name=prefix + "_depthwise_BN")
        self.pointwise_conv = Conv2D(filters, (1, 1), padding="same", use_bias=False, name=prefix + "_pointwise")
        self.pointwise_bn = normalization(name=prefix + "_pointwise_BN")

    def build(self, input_shape):
        # the fused unit reads these layers' weights without calling them: build them from the known widths
        cin = int(input_shape[-1])
        for layer, shape in ((self.depthwise_conv, (1, 1, 1, cin)), (self.depthwise_bn, (1, 1, 1, cin)), (self.pointwise_conv, (1, 1, 1, cin))):
            if not layer.built:
                layer.build(shape)
                layer.built = True
        self.built = True

    def call(self, inputs, training=None):
        if self.activation:
            x = self.depthwise_bn(self.depthwise_conv(inputs), training=training, fused_relu=True)
            x = self.pointwise_bn(self.pointwise_conv(x), training=training, fused_relu=True)
            return x
        dw = self.depthwise_conv
        x = F.sepconv_unit(inputs, dw.depthwise_kernel, self.depthwise_bn, self.pointwise_conv.kernel, training, strides=dw.strides[0],
                           dilation=dw.dilation_rate[0])
        return self.pointwise_bn(x, training=training)

    @property
    def strides(self):
        return self.depthwise_conv.strides

    @strides.setter
    def strides(self, value):
        self.depthwise_conv.strides = _pair(value)

    @property
    def atrous_rates(self):
        return self.depthwise_conv.dilation_rate

    @atrous_rates.setter
    def atrous_rates(self, value):
        self.depthwise_conv.dilation_rate = _pair(value)


class XceptionBlock(Layer):
    def __init__(self, block_index, filters_list, strides, skip_connection=0, activation=False):
        super().__init__(name="block" + str(block_index))
        import torch

        strides = _pair(strides)
        length = len(filters_list)
        self.convs = torch.nn.ModuleList()
        for i in range(length):
            conv_strides = (1, 1) if i < length - 1 else strides
            self.convs.append(XceptionDepthWiseConv(block_index, i + 1, filters_list[i], strides=conv_strides, activation=activation))
        self.skip_connection = skip_connection
        if skip_connection == 2:
            shortcut_name = "block" + str(block_index) + "_shortcut"
            self.shortcut = Conv2D(filters_list[-1], (1, 1), strides=strides, padding="same", use_bias=False, name=shortcut_name)
            self.shortcut_bn = normalization(name=shortcut_name + "_BN")

    def call(self, inputs, training=None):
        if self.skip_connection:
            x, skip = F.fork(inputs, 2)
        else:
            x, skip = inputs, None
        for conv in self.convs:
            x = conv(x, training=training)
        if self.skip_connection == 1:
            x = F.add(x, skip)
        elif self.skip_connection == 2:
            x = F.add(x, self.shortcut_bn(self.shortcut(skip), training=training))
        return x

    @property
    def strides(self):
        return self.convs[-1].strides

    @strides.setter
    def strides(self, value):
        value = _pair(value)
        self.convs[-1].strides = value
        if self.skip_connection == 2:
            self.shortcut.strides = value

    @property
    def atrous_rates(self):
        return self.convs[-1].atrous_rates

    @atrous_rates.setter
    def atrous_rates(self, value):
        value = _pair(value)
        for conv in self.convs:
            conv.atrous_rates = value
        if self.skip_connection == 2:
            self.shortcut.dilation_rate = value      # a 1 x 1 kernel: no effect on the result, kept as the reference sets it


class Xception(Layer):
    def __init__(self, return_endpoints=False, name=None):
        super().__init__(name=name)
        import torch

        self._xception_blocks = torch.nn.ModuleList()
        self.block1_conv1 = Conv2D(32, (3, 3), strides=(2, 2), padding="same", use_bias=False, name="block1_conv1")
        self.block1_conv1_bn = normalization(name="block1_conv1_BN")
        self.block1_conv2 = Conv2D(64, (3, 3), padding="same", use_bias=False, name="block1_conv2")
        self.block1_conv2_bn = normalization(name="block1_conv2_BN")
        self.return_endpoints = return_endpoints

    def call(self, inputs, training=None):
        endpoints = []
        x = self.block1_conv1_bn(self.block1_conv1(F.cast_input(inputs)), training=training, fused_relu=True)
        if self.return_endpoints:
            x, e = F.fork(x, 2)
            endpoints.append(e)
        x = self.block1_conv2_bn(self.block1_conv2(x), training=training, fused_relu=True)
        for block in self._xception_blocks:
            if block.strides[0] > 1 and self.return_endpoints:      # the live stride, after build_atrous_xception
                x, e = F.fork(x, 2)
                endpoints.append(e)
            x = block(x, training=training)
        endpoints.append(x)
        return endpoints if self.return_endpoints else x

    def add_xception_block(self, filters_list, strides, skip_connection=0, activation=False, repeat=1):
        index = len(self._xception_blocks) + 2
        for i in range(repeat):
            self._xception_blocks.append(XceptionBlock(block_index=index + i, filters_list=filters_list, strides=strides,
                                                       skip_connection=skip_connection, activation=activation))

    @property
    def xception_blocks(self):
        return self._xception_blocks


def xception65(return_endpoints=False):
    model = Xception(return_endpoints=return_endpoints, name="xception65")
    model.add_xception_block([128, 128, 128], strides=2, skip_connection=2)      # block 2
    model.add_xception_block([256, 256, 256], strides=2, skip_connection=2)      # block 3
    model.add_xception_block([728, 728, 728], strides=2, skip_connection=2)      # block 4
    model.add_xception_block([728, 728, 728], strides=1, skip_connection=1, repeat=16)      # blocks 5-20: the middle flow
    model.add_xception_block([728, 1024, 1024], strides=2, skip_connection=2)      # block 21
    model.add_xception_block([1536, 1536, 2048], strides=1, skip_connection=0, activation=True)      # block 22
    return model


def build_atrous_xception(model, output_stride=32):
    """once the output stride is reached, every later block runs at stride 1 and the running rate, which grows by the block's stride"""
    current_os = 2
    current_atrous_rates = 1
    for block in model.xception_blocks:
        if current_os >= output_stride:
            block.atrous_rates = (current_atrous_rates, current_atrous_rates)
            current_atrous_rates *= block.strides[0]
            if block.strides[0] > 1:
                block.strides = 1
        else:
            current_os *= block.strides[0]
    return model
