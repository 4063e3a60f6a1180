"""Plain-torch restatement of the reference's DeformableMultiHeadSelfAttentionLayer (layers/deformable_multihead_self_attention.py:89-244), op for
op, so that gradients come from autograd (fp64 in the tests; the dtype follows the inputs).  Test infrastructure only.

    offsets = tanh(offset logits as [N,H,W,heads,P,2]);  dy = [...,0] * (H / orf),  dx = [...,1] * (W / orf)                (:196-207)
    attn    = softmax over P of the attention logits as [N,H,W,heads,P], scrubbed                                            (:210-215)
    y = clip(y_base + dy, 0, H - 1),  x = clip(x_base + dx, 0, W - 1)                                                        (:221-230)
    _bilinear_sample: value as [N*heads, H, W, C_head]; y0 = floor(y), y1 = y0 + 1; INDICES clipped to the image, weights from the
    unclipped y0 (wy1 = y - y0, wy0 = 1 - wy1); four gather_nd with [b, y, x] index triples                                  (:102-174)
    out = sum_p attn_p * sample_p, heads concatenated, scrubbed                                                              (:236-242)

torch.clamp passes the gradient where the input lies inside [min, max], bounds included, as tf.clip_by_value does; floor has none in both.
"""
import torch

EPS = 1e-7      # keras.backend.epsilon()


def replace_nan_or_inf(x, value=EPS):
    """utils/op_utils.py replace_nan_or_inf: non-finite entries become `value` (no gradient through them)"""
    return torch.where(torch.isfinite(x), x, torch.full_like(x, value))


def sampling_coordinates(offset_logits, H, W, heads, points, offset_range_factor):
    """(:196-207, :221-230) -> unclipped (y, x) and clipped (y, x), each [N,H,W,heads,P]"""
    N = offset_logits.shape[0]
    dtype = offset_logits.dtype
    offsets = offset_logits.reshape(N, H, W, heads, points, 2)                          # :197-199
    offset_scale_y = torch.tensor(H / offset_range_factor, dtype=dtype)                 # :203
    offset_scale_x = torch.tensor(W / offset_range_factor, dtype=dtype)                 # :204
    offsets = torch.tanh(offsets)                                                       # :205
    dy = offsets[..., 0] * offset_scale_y                                               # :206
    dx = offsets[..., 1] * offset_scale_x                                               # :207
    y_base = torch.arange(H, dtype=dtype).reshape(1, H, 1, 1, 1).expand(N, H, W, heads, points)      # :91-99
    x_base = torch.arange(W, dtype=dtype).reshape(1, 1, W, 1, 1).expand(N, H, W, heads, points)
    yu = y_base + dy                                                                    # :225
    xu = x_base + dx                                                                    # :226
    y = torch.clamp(yu, 0.0, float(H - 1))                                              # :229
    x = torch.clamp(xu, 0.0, float(W - 1))                                              # :230
    return yu, xu, y, x


def bilinear_sample(value, y, x):
    """_bilinear_sample (:102-174): value [N,H,W,heads,C], y / x [N,H,W,heads,P] -> [N,H,W,heads,P,C]"""
    N, H, W, heads, C = value.shape
    P = x.shape[-1]
    value = value.permute(0, 3, 1, 2, 4)                   # :113
    B = N * heads
    value = value.reshape(B, H, W, C)                      # :115
    y = y.permute(0, 3, 1, 2, 4).reshape(B, H, W, P)       # :118-121
    x = x.permute(0, 3, 1, 2, 4).reshape(B, H, W, P)
    y0 = torch.floor(y)                                    # :124-127
    x0 = torch.floor(x)
    y1 = y0 + 1.0
    x1 = x0 + 1.0
    y0c = torch.clamp(y0.detach().to(torch.int64), 0, H - 1)       # :129-132 (the cast to int cuts the gradient)
    x0c = torch.clamp(x0.detach().to(torch.int64), 0, W - 1)
    y1c = torch.clamp(y1.detach().to(torch.int64), 0, H - 1)
    x1c = torch.clamp(x1.detach().to(torch.int64), 0, W - 1)
    wy1 = y - y0                                           # :134-137
    wx1 = x - x0
    wy0 = 1.0 - wy1
    wx0 = 1.0 - wx1

    def gather_at(y_idx, x_idx):                           # :139-152: gather_nd(value, [b, y, x])
        L = H * W * P
        y_flat = y_idx.reshape(B, L)
        x_flat = x_idx.reshape(B, L)
        b_flat = torch.arange(B).reshape(B, 1).expand(B, L)
        idx = torch.stack([b_flat, y_flat, x_flat], dim=-1).reshape(B * L, 3)
        gathered = value[idx[:, 0], idx[:, 1], idx[:, 2]]
        return gathered.reshape(B, H, W, P, C)

    v00 = gather_at(y0c, x0c)                              # :154-157
    v01 = gather_at(y0c, x1c)
    v10 = gather_at(y1c, x0c)
    v11 = gather_at(y1c, x1c)
    wy0, wy1, wx0, wx1 = (t.unsqueeze(-1) for t in (wy0, wy1, wx0, wx1))      # :159-162
    w00 = wy0 * wx0                                        # :164-167
    w01 = wy0 * wx1
    w10 = wy1 * wx0
    w11 = wy1 * wx1
    out = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11    # :169
    out = out.reshape(N, heads, H, W, P, C)                # :172-173
    return out.permute(0, 2, 3, 1, 4, 5)


def core(value, offset_logits, attn_logits, heads, points, offset_range_factor, scrub=True):
    """(:192-242) behind the projections: value [N,H,W,Cv], offset logits [N,H,W,heads*P*2], attention logits [N,H,W,heads*P] -> [N,H,W,Cv]"""
    N, H, W, Cv = value.shape
    C_head = Cv // heads                                                                # :193
    _, _, y, x = sampling_coordinates(offset_logits, H, W, heads, points, offset_range_factor)
    attn_weights = torch.softmax(attn_logits.reshape(N, H, W, heads, points), dim=-1)   # :211-214 (safed_softmax without a mask)
    attn_weights = replace_nan_or_inf(attn_weights)                                     # :215
    value = value.reshape(N, H, W, heads, C_head)                                       # :219
    sampled = bilinear_sample(value, y, x)                                              # :233
    out = (sampled * attn_weights.unsqueeze(-1)).sum(dim=-2)                            # :236-237
    out = out.reshape(N, H, W, heads * C_head)                                          # :240
    return replace_nan_or_inf(out) if scrub else out                                    # :242


def linear_1x1(x, kernel, bias):
    """keras Conv2D (1, 1) with kernel [1,1,Cin,Cout], or Dense with kernel [Cin,Cout] (:60-64)"""
    return x @ kernel.reshape(kernel.shape[-2], kernel.shape[-1]) + bias


def layer(w, name, query, value, heads, points, offset_range_factor, apply_linear=True):
    """compute_attention_internal (:176-244) with the weights of a layer called `name`; value=None: value = query (:258-259)"""
    if value is None:
        value = query
    query = replace_nan_or_inf(query)                                                   # :182-183
    value = replace_nan_or_inf(value)
    if apply_linear:
        value = linear_1x1(value, w[f"{name}/value_proj/kernel"], w[f"{name}/value_proj/bias"])      # :190
    offsets = linear_1x1(query, w[f"{name}/offset_proj/kernel"], w[f"{name}/offset_proj/bias"])      # :196
    attn_logits = linear_1x1(query, w[f"{name}/attn_proj/kernel"], w[f"{name}/attn_proj/bias"])      # :210
    return core(value, offsets, attn_logits, heads, points, offset_range_factor)
