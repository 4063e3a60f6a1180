"""layers/jpu.py of the reference (:19-90): JointPyramidUpsampling, the FastFCN head piece ("FastFCN: Rethinking Dilated Convolution in the
Backbone for Semantic Segmentation", arXiv 1903.11816).  The last three endpoints each go through a 3x3 ConvNormAct, are resized to the first
one's size and concatenated; the merged map then feeds four separable branches at dilations 1, 2, 4, 8 -- depthwise 3x3 WITH bias (Keras'
DepthwiseConv2D default) -> normalization -> 1x1 ConvNormAct -- whose outputs are concatenated to 4 * width channels.

The four branches read the same tensor: with ISEG_JPU_FUSED=1 (opt-in) F.jpu_tail runs depthwise + BN + pointwise of all four as one tape node
(csrc/jpu.hip) where its predicate allows, else branch by branch on depthwise_conv2d / batch_norm / conv2d."""
import torch

from .. import functional as F
from ..nn import Layer
from ..utils.common import resize_image
from .base_layers import DepthwiseConv2D
from .model_builder import ConvNormAct
from .normalizations import normalization

DILATION_RATES = (1, 2, 4, 8)


class JointPyramidUpsampling(Layer):
    def __init__(self, width=512, trainable=True, name=None):
        super().__init__(trainable=trainable, name=name)
        self.width = width

    def build(self, input_shape):
        endpoints_shape_list = input_shape
        assert len(endpoints_shape_list) >= 3
        base_filters = self.width
        self.endpoints_convs = torch.nn.ModuleList([
            ConvNormAct(base_filters, (3, 3), trainable=self.trainable, name=f"{self.name}/endpoint_conv_{i}") for i in range(3)])
        self.end_depthwise_convs = torch.nn.ModuleList([
            DepthwiseConv2D((3, 3), padding="same", dilation_rate=r, trainable=self.trainable, name=f"{self.name}/end_depthwise_conv_{r}")
            for r in DILATION_RATES])
        self.end_depthwise_bns = torch.nn.ModuleList([
            normalization(trainable=self.trainable, name=f"{self.name}/end_depthwise_bn_{r}") for r in DILATION_RATES])
        self.end_pointwise_convs = torch.nn.ModuleList([
            ConvNormAct(base_filters, trainable=self.trainable, name=f"{self.name}/end_pointwise_convs_{r}") for r in DILATION_RATES])
        self.built = True

    def call(self, inputs, training=None):
        endpoints = list(inputs)
        num_endpoints = len(self.endpoints_convs)
        assert num_endpoints <= len(endpoints)
        endpoints = endpoints[-num_endpoints:]
        size = (endpoints[0].shape[1], endpoints[0].shape[2])
        for i in range(num_endpoints):
            endpoint = self.endpoints_convs[i](endpoints[i], training=training)
            if i > 0:      # (the first one already has the target size: tf.image.resize to the same size is the identity)
                endpoint = resize_image(endpoint, size=size)
            endpoints[i] = endpoint
        merged_features = F.concat(endpoints)
        if self._tail_as_one_node():
            pre = F.jpu_tail(merged_features, list(self.end_depthwise_convs), list(self.end_depthwise_bns),
                             [b.conv.kernel for b in self.end_pointwise_convs], training)
            results = [b.norm_act(v, training=training) for b, v in zip(self.end_pointwise_convs, pre)]
            return F.concat(results)
        results = []
        xs = F.fork(merged_features, len(self.end_depthwise_convs))      # one alias per branch: the branch gradients are summed by our own kernel
        for i in range(len(self.end_depthwise_convs)):
            x = self.end_depthwise_convs[i](xs[i])
            x = self.end_depthwise_bns[i](x, training=training)
            x = self.end_pointwise_convs[i](x, training=training)
            results += [x]
        return F.concat(results)

    def _tail_as_one_node(self):
        """F.jpu_tail takes the branches' variables, so every sub-layer must exist (the first, shape-only call builds them) and be the plain
        kind: BatchNormalization after the depthwise convolution, a bias-free 1x1 Conv2D in the pointwise block"""
        from .. import nn
        from .base_layers import BatchNormalization, Conv2D

        if nn.dry_run():
            return False
        for dw, bn, pw in zip(self.end_depthwise_convs, self.end_depthwise_bns, self.end_pointwise_convs):
            c = pw.conv
            if not (dw.built and bn.built and isinstance(bn, BatchNormalization) and isinstance(c, Conv2D) and c.built and c.bias is None
                    and c.activation is None and c.groups == 1 and c.kernel_size == (1, 1)):
                return False
        return True
