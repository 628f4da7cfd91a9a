// topk_select.h — the order rule and the LDS list sort that the selecting kernels share: the embedding index's (search.hip) and the
// sparse index's (sparse_index.hip).  Device code; a list entry is a (score, id) pair in two parallel LDS arrays, and the workgroup
// has NT threads (search_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

#include "search_kernels.h"

namespace bert_hip {

namespace {

// (s, i) ranks before (ts, ti)
__device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// Sorts nl lists of L (pow2) keys each, best first, with all NT threads of the workgroup.  Enter after a barrier; ends
// with one.
__device__ void bitonic_sort_lists(float *ls, int *li, int nl, int L, int tid) {
    const int lg_half = __builtin_ctz((unsigned)L) - 1, total = nl << lg_half;
    for (int size = 2; size <= L; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int lg_s = __builtin_ctz((unsigned)stride);
            for (int p = tid; p < total; p += NT) {
                const int list = p >> lg_half, i = p & ((1 << lg_half) - 1);
                const int lo = ((i >> lg_s) << (lg_s + 1)) + (i & (stride - 1)), hi = lo + stride;
                float *s = ls + list * L;
                int *d = li + list * L;
                const float sl = s[lo], sh = s[hi];
                const int il = d[lo], ih = d[hi];
                const bool swap = (lo & size) == 0 ? better(sh, ih, sl, il) : better(sl, il, sh, ih);
                if (swap) { s[lo] = sh; s[hi] = sl; d[lo] = ih; d[hi] = il; }
            }
            __syncthreads();
        }
}

}  // namespace

}  // namespace bert_hip
