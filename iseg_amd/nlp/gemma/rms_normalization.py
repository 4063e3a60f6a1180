"""nlp/gemma/rms_normalization.py of the reference (:19-40): x * rsqrt(mean(x^2) + eps) * (1 + scale), statistics in float32, `scale` starts at
zero -- the same operator as layers/rmsnorm.py, whose layer and kernels (iseg_rmsnorm_fwd / _bwd) this one is."""
from ...layers.rmsnorm import RMSNormalization as _RMSNormalization


class RMSNormalization(_RMSNormalization):
    pass
