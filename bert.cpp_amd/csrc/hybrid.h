// hybrid.h — hybrid search: the exact top-k of H = (w_dense * D) + (w_sparse * S) over the rows that are live in an embedding index
// (search.h), live in a sparse index (sparse_index.h) and allowed, D and S being the two indexes' own score bits (hybrid.cpp; C ABI:
// bert_hip_hybrid_* in include/bert_hip.h, hybrid_api.cpp).  Two passes per chunk of queries on the caller's stream: index_scores_kernel
// writes the chunk's dense scores to a matrix [HC][ld] in HBM, sparse_hybrid_scan_kernel reads them while it scans the term rows, and
// selects on chip; topk_merge_kernel merges the slices' lists.  The matrix and the combined bitmap are buffers of the sparse index,
// the lists and query images its existing ones, the dense query buffer the embedding index's.  The call is ONE operation of both
// indexes: it waits for both events and leaves both recorded.
// `inverted` (bert_hip_dense_sparse_search_inverted*): the same chunks, dense pass, bitmap and merge, with the second pass over the
// sparse index's postings — sparse_query_sort_kernel and sparse_postings_hybrid_scan_kernel, which finds S in its LDS accumulators —
// and the same ids and score bits.  It needs postings that cover every row (SparseIndex::invert), else -2.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "search.h"
#include "sparse_index.h"

namespace bert_hip {

// (a friend of both classes; every function: 0, or -2 (refused, nothing changed) or -3 (a device error), a message in err either way)
struct Hybrid {
    // what every entry asks of the pair and the shape: one device, equal sizes, 1 <= k, kq <= 256, finite weights, an allow-list of
    // at least ceil(size / 32) words (n_words is ignored without one).  have_ptrs: every pointer the call needs with n_queries > 0
    // is there; inverted: the sparse index's postings cover its rows.  1 = go on, 0 = nothing to do (n_queries == 0), -2 = refused
    static int check(const Index &d, const SparseIndex &sp, int nq, bool have_ptrs, int kq, float w_dense, float w_sparse, const void *allow,
                     int n_words, int k, std::string &err, bool inverted = false);
    // both indexes' reserve for these bounds, and the hybrid workspace of searches of up to n_queries queries over up to n_rows rows
    static int reserve(Index &d, SparseIndex &sp, int n_rows, int n_queries, int k, std::string &err);
    // everything in device memory, unchecked; asynchronous on s.  The caller has passed check
    static int search_device(Index &d, SparseIndex &sp, int nq, const float *d_q, int kq, const int32_t *d_qids, const float *d_qw, float w_dense,
                             float w_sparse, const uint32_t *d_allow, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                             bool inverted = false);
    // host queries (the sparse ones checked as SparseIndex::search_host checks them), allow-list and results (written only on
    // success); blocking, on the sparse index's stream
    static int search_host(Index &d, SparseIndex &sp, int nq, const float *q, int kq, const int32_t *qids, const float *qw, float w_dense,
                           float w_sparse, const uint32_t *allow, int k, int32_t *ids, float *scores, std::string &err, bool inverted = false);
    // device queries (the text route: the embeddings in the dense index's scratch, the terms in the sparse index's text buffer),
    // host results; blocking, on the sparse index's stream
    static int search_device_to_host(Index &d, SparseIndex &sp, int nq, const float *d_q, int kq, const int32_t *d_qids, const float *d_qw,
                                     float w_dense, float w_sparse, int k, int32_t *ids, float *scores, std::string &err, bool inverted = false);
};

}  // namespace bert_hip
