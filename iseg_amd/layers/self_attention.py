"""layers/self_attention.py of the reference (:15-93): the single-head non-local block.  1x1 query and key projections to `guided_filters`
channels, a 1x1 value projection to `filters` channels, softmax(q k^T [/ sqrt(guided_filters)]) v over all H*W positions with dropout on the
probabilities, reshape back to [N,H,W,filters], feature dropout, optional 1x1 output projection.

Everything between the projections and the feature dropout (:73-85) is F.self_attention_core: with the default widths (64 / 512), bf16 and
no attention dropout in effect it runs on the fused kernels of csrc/selfattn.hip and the [N, HW, HW] probability tensor never exists
(ISEG_SELFATTN_FUSED=0, another width, fp32 or attention dropout in training: the composed route of F.attention_packed).

Deviations: the reference records the attention map with its visualisation manager while that is recording (:55, :78-79); there is no
visualisation manager here and the map is not materialised, so that recording is left out.  With shared_querykey the reference runs the one
projection twice (:69-70); here it runs once and both operands read the same tensor -- the same values, and the projection's gradient is
the sum of the query and the key gradient either way."""
import math

from .. import functional as F
from ..nn import Layer
from . import base_layers


class SelfAttention(Layer):
    def __init__(self, guided_filters=64, filters=512, shared_querykey_weights=False, shared_querykey=False, attention_dropout_rate=0,
                 feature_dropout_rate=0, apply_scale=False, conv_function=base_layers.Conv2D, use_out_projection=False, name=None):
        super().__init__(name=name)
        self.guided_filters, self.filters = guided_filters, filters
        self.shared_querykey_weights, self.shared_querykey = shared_querykey_weights, shared_querykey
        self.attention_dropout_rate, self.feature_dropout_rate = attention_dropout_rate, feature_dropout_rate
        self.apply_scale = apply_scale
        self.use_out_projection = use_out_projection

        def conv(units, name):
            return conv_function(units, 1, kernel_initializer="glorot_uniform", name=f"{self.name}/{name}")

        self.query_conv = conv(guided_filters, "query_conv")
        self.key_conv = self.query_conv if shared_querykey else conv(guided_filters, "key_conv")
        self.value_conv = conv_function(filters, 1, name=f"{self.name}/value_conv")
        self.attention_dropout = base_layers.Dropout(rate=attention_dropout_rate, name=f"{self.name}/attention_dropout")
        self.feature_dropout = base_layers.Dropout(rate=feature_dropout_rate, name=f"{self.name}/feature_dropout")
        if self.use_out_projection:
            self.out_projection = conv(filters, "out_projection")

    def build(self, input_shape):
        if self.shared_querykey_weights and not self.shared_querykey:   # SharedInitializer: the same initial values (:38-40)
            for layer in (self.query_conv, self.key_conv):
                if not layer.built:
                    layer.build(input_shape)
                    layer.built = True
            self.key_conv.kernel.data.copy_(self.query_conv.kernel.data)
        self.built = True

    def call(self, inputs, training=None):
        n, h, w, _ = inputs.shape
        if self.shared_querykey:
            x_q, x_v = F.fork(inputs, 2)
            query, key = F.fork(self.query_conv(x_q, training=training), 2)
        else:
            x_q, x_k, x_v = F.fork(inputs, 3)
            query = self.query_conv(x_q, training=training)
            key = self.key_conv(x_k, training=training)
        value = self.value_conv(x_v, training=training)
        scale = 1.0 / math.sqrt(self.guided_filters) if self.apply_scale else 1.0
        # (:73-85) the attention dropout acts on the probabilities, which only exist inside the core: it gets the layer's rate
        value = F.self_attention_core(query.reshape(n, h * w, query.shape[-1]), key.reshape(n, h * w, key.shape[-1]),
                                      value.reshape(n, h * w, value.shape[-1]), scale, dropout_rate=self.attention_dropout.rate,
                                      training=bool(training))
        value = value.reshape(n, h, w, value.shape[-1])
        value = self.feature_dropout(value, training=training)
        if self.use_out_projection:
            value = self.out_projection(value, training=training)
        return value
