// token_scan_mask.h — the step mask of the token index's masked scans (token_index.hip, token_index_grouped.hip): stated once.  Device code.
#pragma once
#include <hip/hip_runtime.h>

#include "token_index_kernels.h"

namespace bert_hip {

namespace {

static_assert(TOKEN_STEP_DOCS == 64, "the masked scan keeps a step's mask in one 64-bit word");

// the word of live & allow (a null pointer: all ones) at index wi, the same in every lane
__device__ __forceinline__ uint32_t token_mask_word(const TokenScanArgs &a, int wi) {
    uint32_t w = ~0u;
    if (a.live) w &= a.live[wi];
    if (a.allow) w &= a.allow[wi];
    return __builtin_amdgcn_readfirstlane(w);
}

// Bit i of the result = document base + i qualifies.  The step's documents lie in up to three mask words (a slice starts anywhere);
// only words that hold a document below r1 are read, so none at or beyond ceil(n_docs / 32).  Everything here is computed from the
// workgroup's values alone, the same in all four waves.
__device__ __forceinline__ uint64_t token_step_mask(const TokenScanArgs &a, int base, int r1) {
    const int wi = base >> 5, sh = base & 31, we = (min(base + TOKEN_STEP_DOCS, r1) - 1) >> 5;
    const uint32_t w0 = token_mask_word(a, wi);
    const uint32_t w1 = wi + 1 <= we ? token_mask_word(a, wi + 1) : 0u;
    const uint32_t w2 = wi + 2 <= we ? token_mask_word(a, wi + 2) : 0u;
    uint64_t m = ((uint64_t)w1 << 32 | w0) >> sh;
    if (sh) m |= (uint64_t)w2 << (64 - sh);
    return m;
}

}  // namespace

}  // namespace bert_hip
