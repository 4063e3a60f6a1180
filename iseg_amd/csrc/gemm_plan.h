// How a reduction is cut into split-K slabs: the one place that turns (K, splits asked for) into the numbers every GEMM-family launcher and
// workspace query needs.  The split POLICIES stay with their families -- choose_split (gemm.hip) and conv_splits (conv_igemm.hip) -- and feed it.
#pragma once
#include "common.h"

namespace iseg_mm {

struct SplitPlan {
    int nsplit;             // splits the policy asked for: the slab buffer is sized for these
    int64_t kps;            // K elements per split, a multiple of the granule (K itself when unsplit)
    int eff_split;          // slabs really written, ceil(K / kps) <= nsplit: grid.y of the main loop, what the reducer sums
    int64_t slab_rows;      // rows of one slab (M, + 1 with the ones-row of a bias gradient)
    size_t slab_bytes;      // nsplit slabs of slab_rows x N floats; 0 when unsplit
};

// granule: 128 for iseg_gemm and the patch-view weight gradient, 64 for the implicit-GEMM convolutions
inline SplitPlan split_plan(int64_t K, int nsplit, int granule, int64_t rows, int64_t N) {
    SplitPlan p{nsplit, K, 1, rows, 0};
    if (nsplit > 1) {
        p.kps = ceil_div64(ceil_div64(K, nsplit), granule) * granule;
        if (p.kps > 0) p.eff_split = (int)ceil_div64(K, p.kps);
        p.slab_bytes = (size_t)nsplit * (size_t)rows * (size_t)N * sizeof(float);
    }
    return p;
}

}  // namespace iseg_mm
