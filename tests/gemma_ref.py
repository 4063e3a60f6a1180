"""fp64 torch restatement of the reference's Gemma backbone, the yardstick of tests/test_gemma_host.py and tests/test_gemma_gpu.py:
nlp/gemma/rms_normalization.py, gemma_attention.py, gemma_decoder_block.py and gemma_backbone.py, line by line.  Test infrastructure only.

Weights are a dict name -> tensor with the reference's variable names (gemma_backbone.py:231-243)."""
import math

import torch

LARGE_NEGATIVE = -1e9      # keras.layers.Softmax(mask=): inputs += (1 - mask) * -1e9


def rms_norm(x, scale, eps):
    """rms_normalization.py:33-40"""
    var = x.pow(2).mean(-1, keepdim=True)
    return x * torch.rsqrt(var + eps) * (1 + scale)


def gelu_tanh(x):
    """keras.activations.gelu(approximate=True) (gemma_decoder_block.py:171)"""
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x.pow(3))))


def gelu_tanh_grad(x):
    u = math.sqrt(2 / math.pi) * (x + 0.044715 * x.pow(3))
    t = torch.tanh(u)
    sech2 = torch.where(u.abs() > 300, torch.zeros_like(u), 1 - t * t)
    inner = torch.where(sech2 == 0, torch.zeros_like(u), 0.5 * x * sech2 * math.sqrt(2 / math.pi) * (1 + 3 * 0.044715 * x * x))
    return 0.5 * (1 + t) + inner


def apply_rope(x, positions):
    """gemma_attention.py:96-114 -- x [B, T, N, h], positions [T]; the output is the stack of the two expressions along a NEW last axis,
    reshaped to h: element 2i is x1 cos - x2 sin, element 2i + 1 is x2 cos + x1 sin"""
    h = x.shape[-1]
    freq_exponents = (2.0 / h) * torch.arange(h // 2, dtype=x.dtype)
    timescale = 10000.0 ** freq_exponents
    radians = positions[..., None] / timescale[None, None, :]      # [1, T, h/2]
    radians = radians[..., None, :]                                 # [1, T, 1, h/2]
    sin, cos = torch.sin(radians), torch.cos(radians)
    x1, x2 = torch.split(x, h // 2, dim=-1)
    output = torch.stack([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    return output.reshape(x.shape)


def attention_mask(padding_mask, B, T):
    """gemma_decoder_block.py:114-136 -- bool [B, T, T]: minimum(padding mask over the keys, causal mask)"""
    causal = torch.ones(T, T, dtype=torch.bool).tril()[None].expand(B, T, T)
    if padding_mask is None:
        return causal
    return causal & (padding_mask.reshape(B, 1, T) != 0)


def compute_attention(q, k, v, mask, nq, nkv):
    """gemma_attention.py:116-151 -- q [B, T, nq, h], k, v [B, T, nkv, h], mask bool [B, T, T] -> [B, T, nq, h]"""
    B, T, _, h = q.shape
    q = q * (1 / math.sqrt(h))
    q = q.reshape(B, T, nkv, nq // nkv, h)
    logits = torch.einsum("btkgh,bskh->bkgts", q, k)
    m = mask[:, None, None, :, :]
    logits = logits + (1.0 - m.to(logits.dtype)) * LARGE_NEGATIVE
    p = torch.softmax(logits, dim=-1)
    results = torch.einsum("bkgts,bskh->btkgh", p, v)
    return results.reshape(B, T, nq, h)


def wipe(vec, mask):
    """gemma_attention.py:189-195 -- rows without an attended token become zeros (tf.where: no gradient flows into them)"""
    none = ~mask.any(dim=-1, keepdim=True)[..., None]      # [B, T, 1, 1]
    return torch.where(none, torch.zeros_like(vec), vec)


def attention_core(q, k, v, padding_mask, nq, nkv):
    """what F.gemma_attention_core computes: q, k already rotated; -> [B, T, nq * h]"""
    B, T = q.shape[:2]
    mask = attention_mask(padding_mask, B, T)
    return wipe(compute_attention(q, k, v, mask, nq, nkv), mask).reshape(B, T, -1)


def attention(x, w, prefix, padding_mask, nq, nkv):
    """CachedGemmaAttention.call without a cache (gemma_attention.py:153-201)"""
    B, T, _ = x.shape
    positions = torch.arange(T, dtype=x.dtype)[None]
    q = apply_rope(torch.einsum("btd,ndh->btnh", x, w[prefix + "query/kernel"]), positions)
    k = apply_rope(torch.einsum("bsd,kdh->bskh", x, w[prefix + "key/kernel"]), positions)
    v = torch.einsum("bsd,kdh->bskh", x, w[prefix + "value/kernel"])
    mask = attention_mask(padding_mask, B, T)
    vec = wipe(compute_attention(q, k, v, mask, nq, nkv), mask)
    return torch.einsum("btnh,nhd->btd", vec, w[prefix + "attention_output/kernel"])


def decoder_block(x, w, prefix, padding_mask, nq, nkv, eps=1e-6):
    """GemmaDecoderBlock.call (gemma_decoder_block.py:139-178)"""
    normalized = rms_norm(x, w[prefix + "pre_attention_norm/scale"], eps)
    attention_x = x + attention(normalized, w, prefix + "attention/", padding_mask, nq, nkv)
    normalized = rms_norm(attention_x, w[prefix + "pre_ffw_norm/scale"], eps)
    x1 = normalized @ w[prefix + "ffw_gating/kernel"]
    x2 = normalized @ w[prefix + "ffw_gating_2/kernel"]
    return (gelu_tanh(x1) * x2) @ w[prefix + "ffw_linear/kernel"] + attention_x


def backbone(token_ids, padding_mask, w, num_layers, nq, nkv, eps=1e-6, act_dtype=torch.float32):
    """GemmaBackbone (gemma_backbone.py:152-156); sqrt(hidden_dim) is rounded to the activation type before the product (:153)"""
    table = w["token_embedding/embeddings"]
    x = table[token_ids.long()]
    x = x * float(torch.tensor(math.sqrt(float(table.shape[1])), dtype=torch.float32).to(act_dtype))
    for i in range(num_layers):
        x = decoder_block(x, w, f"decoder_block_{i}/", padding_mask, nq, nkv, eps)
    return rms_norm(x, w["final_normalization/scale"], eps)
