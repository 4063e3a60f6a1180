"""nlp/gemma/ of the reference: the Gemma text backbone (decoder-only transformer: RMS normalisation, rotary embedding, causal grouped-query
attention, GeGLU feed-forward).  Built here: the backbone and its layers, the logits of the tied embedding, GemmaCausalLM with its KV cache,
greedy generation and scoring.  Not built: the tokenizer and preprocessors, preset download, samplers other than greedy, get_layout_map."""
from .gemma_attention import CachedGemmaAttention  # noqa: F401
from .gemma_backbone import GemmaBackbone  # noqa: F401
from .gemma_causal import GemmaCausalLM  # noqa: F401
from .gemma_decoder_block import GemmaDecoderBlock  # noqa: F401
from .rms_normalization import RMSNormalization  # noqa: F401
