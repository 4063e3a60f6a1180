// bf16 MFMA GEMM instantiations, orientation "nn" (see gemm_impl.h); split from gemm.hip for parallel compilation.
#include "gemm_impl.h"

namespace iseg_mm {
void gemm_bf16_nn(const iseg_gemm_args* g, const Epi& epi, const SplitPlan& p, float* slabs, hipStream_t s) {
    if (g->out_dtype == ISEG_BF16) dispatch_bk<true, false, bf16_t>(g, epi, p.eff_split, p.kps, slabs, s);
    else dispatch_bk<true, false, float>(g, epi, p.eff_split, p.kps, slabs, s);
}
}  // namespace iseg_mm
