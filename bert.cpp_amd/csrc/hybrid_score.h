// hybrid_score.h — the hybrid score of bert_hip.h ("Hybrid search"), for the two scan kernels that select by it:
// sparse_hybrid_scan_kernel (sparse_index.hip, over the rows) and sparse_postings_hybrid_scan_kernel (sparse_postings.hip, over the
// postings).  One text, so that both give a (D, S) pair the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace bert_hip {

// The hybrid score H = (w_dense * D) + (w_sparse * S) of bert_hip.h: two f32 multiplications and one f32 addition, each rounded to
// nearest even, never an fma (contraction is off for this block, whatever the translation unit's default)
__device__ __forceinline__ float hybrid_score(float w_dense, float d, float w_sparse, float s) {
#pragma clang fp contract(off)
    const float x = w_dense * d;
    const float y = w_sparse * s;
    return x + y;
}

}  // namespace bert_hip
