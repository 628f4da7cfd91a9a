// topk_select.h — the selection every search ends in: the order rule, the LDS list sort and the queue around it (DESIGN.md §8.1
// describes the protocol).  index_probe_kernel, topk_merge_kernel (search.hip), the postings scan body (sparse_postings.hip) and
// token_index_scan_kernel (token_index.hip) use the helpers; index_topk_kernel and the row-major sparse_scan_body follow the same
// protocol with its lines written out, because through the helpers they measured slower (§8.1).  Device code, NT threads a workgroup.
//
// nl lists of L (pow2) (score, id) entries and a count each, in LDS: list q's top-k sorted in [0, k), its queue behind; a lane
// pushes what beats its register copy of the threshold (entry k - 1 as of the last sort); room = L - k - (the most pushes of a
// step); an empty entry is (-inf, SENT_ID).  Every thread of the workgroup calls select_init, select_step_end, select_resume and
// select_finish, with trip counts that are the workgroup's:
//   select_init      the caller's barrier follows, in front of the first push.
//   select_step_end  entered after the step's pushes.  The look — thread q reads count q; one list (nl a literal 1): thread 0, at
//                    a uniform address — has a barrier on either side.  False: nothing changed, nothing owed.  True: the lists
//                    are sorted and the counts are STILL the step's; the caller reloads its thresholds and then MUST call
//   select_resume    which zeroes the counts and holds the ONE barrier that lets the next step push.  Without it the code
//                    compiles, the counts grow on and the next pushes run past the list.
//   select_finish    entered after the last step; ends with a barrier: [0, k) of every list may then be read by any thread.
// The order of the statements in select_init, select_threshold and select_resume holds register counts and a loop offset (§8.1).
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "search_kernels.h"

namespace bert_hip {

namespace {

constexpr int SENT_ID = INT_MAX;        // id of an empty list entry (score -inf): ranks below every row or document

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

// the lists of one workgroup: scores [nl][L], ids [nl][L], counts [nl] in LDS
struct SelectLists { float *ls; int *li; int *cnt; int L, k, room; };

__device__ __forceinline__ void select_init(const SelectLists &sel, int nl, int tid) {
    for (int i = tid; i < nl * sel.L; i += NT) { sel.ls[i] = -INFINITY; sel.li[i] = SENT_ID; }
    if (tid < nl) sel.cnt[nl == 1 ? 0 : tid] = 0;
}

__device__ __forceinline__ void select_push(const SelectLists &sel, int q, float s, int id) {
    const int p = atomicAdd(&sel.cnt[q], 1);
    sel.ls[q * sel.L + sel.k + p] = s;
    sel.li[q * sel.L + sel.k + p] = id;
}

__device__ __forceinline__ bool select_step_end(const SelectLists &sel, int nl, int tid) {
    __syncthreads();
    if (!__syncthreads_or(tid < nl && sel.cnt[nl == 1 ? 0 : tid] > sel.room)) return false;
    bitonic_sort_lists(sel.ls, sel.li, nl, sel.L, tid);
    return true;
}

// list q's threshold: its k-th best as of the last sort
__device__ __forceinline__ void select_threshold(const SelectLists &sel, int q, float &ts, int &ti) {
    const float s = sel.ls[q * sel.L + sel.k - 1];
    const int i = sel.li[q * sel.L + sel.k - 1];
    ts = s; ti = i;
}

__device__ __forceinline__ void select_resume(const SelectLists &sel, int nl, int tid) {
    if (tid < nl) sel.cnt[nl == 1 ? 0 : tid] = 0;
    __syncthreads();
}

__device__ __forceinline__ void select_finish(const SelectLists &sel, int nl, int tid) {
    __syncthreads();
    if (__syncthreads_or(tid < nl && sel.cnt[nl == 1 ? 0 : tid] > 0)) bitonic_sort_lists(sel.ls, sel.li, nl, sel.L, tid);
}

// [0, k) of list q -> the workspace's list of (query q0 + q, slice): ws [queries][n_slices][k]
__device__ __forceinline__ void select_store(const SelectLists &sel, int nl, float *ws_s, int *ws_i, int q0, int n_slices, int slice, int tid) {
    const int k = sel.k;
    for (int i = tid; i < nl * k; i += NT) {
        const int q = i / k, j = i - q * k;
        const size_t o = ((size_t)(q0 + q) * n_slices + slice) * k + j;
        ws_s[o] = sel.ls[q * sel.L + j];
        ws_i[o] = sel.li[q * sel.L + j];
    }
}

// the k entries at ws + out of a (query, slice) without a candidate
__device__ __forceinline__ void select_store_empty(float *ws_s, int *ws_i, size_t out, int k, int tid) {
    for (int j = tid; j < k; j += NT) { ws_s[out + j] = -INFINITY; ws_i[out + j] = SENT_ID; }
}

}  // namespace

}  // namespace bert_hip
