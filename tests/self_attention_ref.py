"""Plain-torch restatement of the reference's SelfAttention (layers/self_attention.py:65-93) and of get_attention
(utils/attention_utils.py:23-40), op for op, so that gradients come from autograd (fp64 in the tests; the dtype follows the inputs).
Test infrastructure only.

    query = query_conv(x), key = key_conv(x), value = value_conv(x)                                    (:69-71)
    query = flatten_hw(query); key = transpose_hw_c(flatten_hw(key))                                   (:73-74)
    attention = softmax(query @ key [/ sqrt(query.shape[-1])])                                         (:76, attention_utils.py:30-35)
    value = attention_dropout(attention) @ flatten_hw(value), reshaped to [N,H,W,filters]              (:81-86)
    value = feature_dropout(value); value = out_projection(value) when use_out_projection              (:88-91)

Both dropouts are identities here (training=False, or a rate of 0); the recording of the attention map (:78-79) has no effect on the result.
"""
import math

import torch


def flatten_hw(x):
    """utils/attention_utils.py:11-15"""
    return x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[-1])


def transpose_hw_c(x):
    """utils/attention_utils.py:18-20"""
    return x.permute(0, 2, 1)


def get_attention(query, key, apply_scale=False):
    """utils/attention_utils.py:23-40 (numeric_stable only changes the dtype of the same operations): query [N,T,C], key [N,C,T]"""
    x = torch.matmul(query, key)                                                        # :30
    if apply_scale:
        x = x / math.sqrt(query.shape[-1])                                              # :33
    return torch.softmax(x, dim=-1)                                                     # :35


def core(query, key, value, scale):
    """softmax(scale * q k^T) v on flattened operands [B,T,dk], [B,T,dk], [B,T,dv] -- lines :74-85 with an explicit factor"""
    x = torch.matmul(query, transpose_hw_c(key)) * scale
    return torch.matmul(torch.softmax(x, dim=-1), value)


def linear_1x1(x, kernel, bias):
    """keras Conv2D (1, 1) with kernel [1,1,Cin,Cout]"""
    return x @ kernel.reshape(kernel.shape[-2], kernel.shape[-1]) + bias


def layer(w, name, inputs, shared_querykey=False, apply_scale=False, use_out_projection=False):
    """SelfAttention.call (:65-93) with the weights of a layer called `name`; with shared_querykey the key projection IS the query
    projection (:46-47)"""
    batch_size, height, width, _ = inputs.shape                                         # :67
    key_name = "query_conv" if shared_querykey else "key_conv"
    query = linear_1x1(inputs, w[f"{name}/query_conv/kernel"], w[f"{name}/query_conv/bias"])      # :69
    key = linear_1x1(inputs, w[f"{name}/{key_name}/kernel"], w[f"{name}/{key_name}/bias"])        # :70
    value = linear_1x1(inputs, w[f"{name}/value_conv/kernel"], w[f"{name}/value_conv/bias"])      # :71
    query = flatten_hw(query)                                                           # :73
    key = transpose_hw_c(flatten_hw(key))                                               # :74
    attention = get_attention(query, key, apply_scale=apply_scale)                      # :76
    value = flatten_hw(value)                                                           # :81
    value = torch.matmul(attention, value)                                              # :85
    value = value.reshape(batch_size, height, width, value.shape[-1])                   # :86
    if use_out_projection:
        value = linear_1x1(value, w[f"{name}/out_projection/kernel"], w[f"{name}/out_projection/bias"])      # :90-91
    return value
