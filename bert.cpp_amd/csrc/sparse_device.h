// sparse_device.h — what the sparse index's two device units (sparse_index.hip, sparse_postings.hip) share: the stored types, the
// map between a row's column and its storage slot (sparse_index_kernels.h states the stored form), the rank-by-count of a row's or
// a query's terms, and the launch of a <DTYPE, MASKED> scan family.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <initializer_list>
#include <type_traits>

#include "kernels.h"
#include "sparse_index_kernels.h"

namespace bert_hip {

namespace {

template <int DTYPE> struct Stored {
    using id_t = std::conditional_t<DTYPE == 1, uint16_t, int32_t>;
    using w_t = std::conditional_t<DTYPE == 1, half_t, float>;
};

// element (row, column j) of a stored array of rows `width` columns wide
__device__ __forceinline__ size_t slot(int row, int j, int width) {
    return ((size_t)(row >> 6) * width + j) * SPARSE_BLOCK_ROWS + (row & 63);
}
// slot()'s inverse: storage slot e is column (e / 64) % width of row (e / (64 * width)) * 64 + e % 64
__device__ __forceinline__ void slot_decode(size_t e, int width, int &row, int &j) {
    const size_t per_block = (size_t)width * SPARSE_BLOCK_ROWS, blk = e / per_block;
    const int in = (int)(e - blk * per_block);
    j = in >> 6; row = (int)blk * SPARSE_BLOCK_ROWS + (in & 63);
}
// the slots of the blocks that n rows take
__host__ __device__ inline size_t block_slots(int n, int width) {
    return (size_t)((n + SPARSE_BLOCK_ROWS - 1) / SPARSE_BLOCK_ROWS) * width * SPARSE_BLOCK_ROWS;
}

// Rank-by-count over one workgroup of SPARSE_MAX_TERMS threads: thread t < n_in offers entry first + t of ids / weights; an id
// outside [0, n_vocab) is dropped (key INT_MAX, weight +0).  rank: the entry's place among the kept ones by (id, input position) —
// every kept entry has a rank of its own below count <= n_in.  keys: SPARSE_MAX_TERMS ints of LDS; holds a barrier.
struct RankedTerm { int key; float w; int rank, count; };
__device__ __forceinline__ RankedTerm rank_terms(const int32_t *ids, const float *weights, size_t first, int n_in, int n_vocab, int *keys, int t) {
    int key = INT_MAX;
    float w = 0.f;
    if (t < n_in) {
        const int id = ids[first + t];
        if (id >= 0 && id < n_vocab) { key = id; w = weights[first + t]; }
    }
    keys[t] = key;
    const int count = __syncthreads_count(key != INT_MAX);
    int rank = 0;
    if (key != INT_MAX)
        for (int u = 0; u < n_in; ++u) {
            const int ku = keys[u];
            rank += (ku < key || (ku == key && u < t)) ? 1 : 0;
        }
    return RankedTerm{key, w, rank, count};
}

// SPARSE_LDS_MAX of dynamic LDS for the listed kernels, once per device (a launch that still cannot have it fails, and the search reports it)
inline void scan_lds_opt_in(DeviceFlags &seen, std::initializer_list<const void *> kernels) {
    configure_once(seen, [&] {
        bool ok = true;
        for (const void *f : kernels) ok = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPARSE_LDS_MAX) == hipSuccess && ok;
        if (!ok) (void)hipGetLastError();                      // (not left behind for an unrelated call's check)
    });
}

}  // namespace

// the four instantiations of a scan family KERNEL<DTYPE, MASKED>; the launch of the one that (dtype, a.live || a.allow) names
#define SPARSE_SCAN_FAMILY(KERNEL) (const void *)KERNEL<0, false>, (const void *)KERNEL<1, false>, (const void *)KERNEL<0, true>, (const void *)KERNEL<1, true>
#define SPARSE_SCAN_LAUNCH(KERNEL, dtype, a, lds, s)                                                      \
    do {                                                                                                  \
        const dim3 grid_(xcd_grid((a).n_items));                                                          \
        const bool masked_ = (a).live || (a).allow;                                                       \
        if ((dtype) == 1 && masked_) BERT_LAUNCH((KERNEL<1, true>), grid_, dim3(NT), lds, s, a);          \
        else if ((dtype) == 1) BERT_LAUNCH((KERNEL<1, false>), grid_, dim3(NT), lds, s, a);               \
        else if (masked_) BERT_LAUNCH((KERNEL<0, true>), grid_, dim3(NT), lds, s, a);                     \
        else BERT_LAUNCH((KERNEL<0, false>), grid_, dim3(NT), lds, s, a);                                 \
    } while (0)

}  // namespace bert_hip
