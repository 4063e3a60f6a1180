"""layers/deformable_multihead_self_attention.py of the reference (:13-260): per head and per sampling point a tanh-bounded 2-D offset and an
attention logit are predicted from the query (two 1x1 projections); the (optionally projected) value map is sampled bilinearly at the clipped
positions around every pixel and the samples are summed with the softmax of the logits.  There is no query, key or output projection.

Everything between the projections and the output -- tanh, scaling, softmax, clip, the four gathers, the weighted sum (:195-240) -- is one kernel
each way (F.deformable_attention_core, csrc/defattn.hip), with coordinates and weights in fp32 whatever the storage dtype.  The reference's NaN scrub
of the softmax weights (:215) is an identity on finite values and is not materialised (documented deviation for non-finite inputs only, as in
multihead_self_attention.py); the scrubs of query, value and output (:182-183, :242) are kept."""
from .. import functional as F
from ..nn import Layer
from .base_layers import Conv2D, Dense

EPSILON = 1e-7   # keras.backend.epsilon()


class DeformableMultiHeadSelfAttentionLayer(Layer):
    def __init__(self, filters=-1, num_heads=4, num_points=4, apply_linear=True, shared_qk=False, trainable=True, use_dense_for_linear=False,
                 offset_range_factor=8.0, use_jit_compile=False, name=None):
        super().__init__(trainable=trainable, name=name)
        self.filters, self.num_heads, self.num_points = filters, num_heads, num_points
        self.apply_linear = apply_linear
        self.shared_qk = shared_qk                  # (kept for API symmetry by the reference; unused there as well)
        self.use_dense_for_linear = use_dense_for_linear
        self.offset_range_factor = float(offset_range_factor)
        self.use_jit_compile = use_jit_compile      # (XLA switch of the reference: nothing to switch here)
        self.value_proj = self.offset_proj = self.attn_proj = None

    def _make_linear_1x1(self, out_channels, name):
        if self.use_dense_for_linear:
            return Dense(out_channels, trainable=self.trainable, name=f"{self.name}/{name}")
        return Conv2D(out_channels, (1, 1), trainable=self.trainable, name=f"{self.name}/{name}")

    def build(self, input_shape):
        channels = int(input_shape[-1])
        value_filters = channels if self.filters == -1 else int(self.filters)
        if value_filters % self.num_heads != 0:
            raise ValueError(f"value filters ({value_filters}) must be divisible by num_heads ({self.num_heads}).")
        self.value_filters = value_filters
        if self.apply_linear:
            self.value_proj = self._make_linear_1x1(value_filters, "value_proj")
        self.offset_proj = self._make_linear_1x1(self.num_heads * self.num_points * 2, "offset_proj")
        self.attn_proj = self._make_linear_1x1(self.num_heads * self.num_points, "attn_proj")
        self.built = True

    def compute_attention(self, query, value=None):
        """(:176-244) value=None: the query is the value (one scrub, as both scrubs see the same tensor)"""
        query = F.replace_nan_or_inf(query, EPSILON)
        if value is None:
            q_off, q_attn, value = F.fork(query, 3)
        else:
            q_off, q_attn = F.fork(query, 2)
            value = F.replace_nan_or_inf(value, EPSILON)
        if self.apply_linear:
            value = self.value_proj(value)
        out = F.deformable_attention_core(value, self.offset_proj(q_off), self.attn_proj(q_attn), self.num_heads, self.num_points,
                                          self.offset_range_factor)
        return F.replace_nan_or_inf(out, EPSILON)

    def call(self, inputs, key=None, value=None, training=None):
        # (:256-260) `key` is accepted and unused, as in the reference
        return self.compute_attention(inputs, value)
