// sparse_index.h — a sparse index in HBM and its exact top-k inner-product search (the class: sparse_index.cpp; its kernels:
// sparse_index.hip behind sparse_index_kernels.h; C ABI: bert_hip_sparse_index_* in include/bert_hip.h).  Rows are sets of
// (vocabulary id, weight) terms, at most `width` each, on the device of the engine the index was made from, as i32 ids + f32 weights
// or as u16 ids + f16 weights (RNE), in blocks of 64 rows stored column by column (sliced ELL).  A search turns each query into an
// image the scan reads from LDS (sparse_query_kernel), scans the blocks with one row per lane and selects on chip
// (sparse_index_scan_kernel: a top-k per (query, slice of rows) in LDS), and merges the slices' lists per query with the embedding
// index's topk_merge_kernel.  Grow-only storage and workspace; the event, the stream of the host routes and the removed-rows bitmap
// are the frame's that all three indexes derive from (index_frame.h; the bitmap's invariant: live_bits.h).  The bitmap is there from the
// first remove to the next compact; while it exists, or under an allow-list, a search launches the masked scan.  rescore scores per-query candidate rows (sparse_index_rescore_kernel).
// Postings (sparse_postings.cpp, kernels in sparse_postings.hip): invert builds a term-major image of the rows, and the searches'
// `inverted` form answers from it with the row-major search's ids and score bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "engine.h"
#include "index_frame.h"
#include "sparse_index_file.h"
#include "sparse_index_kernels.h"

namespace bert_hip {

class SparseIndex : private IndexFrame {
public:
    static constexpr int MAX_K = 256, MAX_TERMS = SPARSE_MAX_TERMS, MAX_VOCAB = SPARSE_MAX_VOCAB, MAX_CAND = SPARSE_MAX_CAND;
    static constexpr int QCHUNK = 4096;                  // queries per internal pass (workspace and image-buffer bound)

    // dtype 0: i32 ids + f32 weights, 1: u16 ids + f16 weights (n_vocab <= 65536)
    static SparseIndex *create(Engine *eng, int n_vocab, int width, int dtype, std::string &err);
    ~SparseIndex();

    int size() const { return n_; }
    int n_live() const { return n_ - bits_.n_removed; }
    int n_vocab() const { return n_vocab_; }
    int width() const { return width_; }
    int dtype() const { return dtype_; }
    hipStream_t stream() const { return stream_; }

    // Results: >= 0, or -2 (an argument the entry refuses; nothing changed) or -3 (a device error), a message in err either way.
    // storage for n_rows rows and the workspace of searches of up to n_queries queries with any k' <= k, now
    int reserve(int n_rows, int n_queries, int k, std::string &err);
    // append rows ids / weights [n][k_in] in device memory, unchecked (sparse_index_kernels.h): the first new id.  Asynchronous on s
    int add_device(int n, int k_in, const int32_t *d_ids, const float *d_weights, hipStream_t s, std::string &err);
    // host rows, checked (ids in [-1, n_vocab), no id twice in a row, weights finite as stored); blocking
    int add_host(int n, int k_in, const int32_t *ids, const float *weights, std::string &err);
    // ids / scores [nq][k], best first; queries ids / weights [nq][kq] in device memory, unchecked.  Asynchronous on s
    // d_allow: null, or device words [ceil(size / 32)], bit set = the row may be returned
    // inverted: answer from the postings (sparse_postings_scan_kernel) — the same ids and score bits; -2 where the postings do not
    // cover the rows (no invert yet, or rows added since)
    int search_device(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                      const uint32_t *d_allow = nullptr, bool inverted = false);
    // host queries, checked as add_host's rows (weights finite as f32), and host results (written only on success); blocking.  allow:
    // null, or host words as d_allow
    int search_host(int nq, int kq, const int32_t *qids, const float *qw, int k, int32_t *ids, float *scores, std::string &err,
                    const uint32_t *allow = nullptr, bool inverted = false);
    // Per query its n_cand candidate rows d_cand [nq][n_cand] (ids outside [0, size) and removed rows: no candidate) scored with the
    // search's bits, the best k to d_ids / d_scores [nq][k].  1 <= n_cand <= 1024; the workspace [chunk][n_cand] grows on demand and is
    // not part of reserve: call once at the largest shape before a capture.  Asynchronous on s
    int rescore_device(int nq, int kq, const int32_t *d_qids, const float *d_qw, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids,
                       float *d_scores, hipStream_t s, std::string &err);
    // host queries (checked as search_host's), candidates (each in [-1, size), -2 otherwise) and results; blocking
    int rescore_to_host(int nq, int kq, const int32_t *qids, const float *qw, int n_cand, const int32_t *cand, int k, int32_t *ids, float *scores,
                        std::string &err);
    // Removed rows: the number newly removed (repeats and removed rows are ignored); an id outside [0, size): -2, nothing changed.  Blocking
    int remove(int n, const int32_t *ids, std::string &err);
    // Drops the removed rows: the live ones keep their order and bits and get ids 0 .. n_live - 1; old_ids (nullable) [n_live] receives
    // their former ids.  The new size; the bitmap is gone afterwards.  Blocking
    int compact(int32_t *old_ids, std::string &err);
    // the file form (sparse_index_file.h); blocking.  load: from f, positioned behind the header h that sparse_index_header_check passed
    bool save(const char *path, std::string &err);
    static SparseIndex *load(Engine *eng, FILE *f, const SparseIndexFileHeader &h, std::string &err);
    // the live words of the host mirror (live_bits.h: as long as the capacity, bits at and beyond size zero); empty without removals
    const std::vector<uint32_t> &live_words_host() const { return bits_.words; }
    // the stored rows row_ids [n] (each in [0, size)) as out_ids / out_weights [n][width]; blocking
    int get_rows(int n, const int32_t *row_ids, int32_t *out_ids, float *out_weights, std::string &err);
    // Text routes: device buffers of the index for a group's packed token ids | cu_seqlens (in) and its terms ids | weights [n][k] (out);
    // the index's operations that read them are finished
    bool text_buffers(size_t in_bytes, size_t out_bytes, char *&d_in, char *&d_out, std::string &err);
    // the results of a device search of nq queries on stream(), d_ids / d_scores in the index's result buffers -> host; blocking
    int search_device_to_host(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *ids, float *scores, std::string &err,
                              const uint32_t *d_allow = nullptr, bool inverted = false);
    // forget the rows behind the first n (an add of several parts that failed part way)
    void truncate(int n);
    // Postings (sparse_index_kernels.h "Postings and the inverted search"): builds the term-major image of all size() rows from the
    // stored blocks, in segments of the tuning key "sparse_index_segment_rows" (read here), and grows the search workspace to what
    // the inverted plan needs for the n_queries and k last given to reserve.  Every call rebuilds all segments.  Returns the rows
    // covered (= size).  Blocking; allocates
    int invert(std::string &err);
    // rows the postings cover: 0 without postings (never built, dropped by compact, a loaded index)
    int inverted_rows() const { return inverted_ ? inv_rows_ : 0; }
    bool has_postings() const { return inverted_; }
    int segment_rows() const { return inv_seg_; }
    // test hook: segment sg's offsets [n_vocab + 1] and its postings (row number inside the segment, weight as f32 — exact), in slot
    // order, to the host; the segment's term total, -2 without postings or for a segment they do not have.  Blocking
    int postings_segment_host(int sg, std::vector<uint32_t> &off, std::vector<uint16_t> &rows, std::vector<float> &weights, std::string &err);

private:
    friend struct Hybrid;                               // hybrid.h: a search over this index and an embedding index together
    SparseIndex() = default;
    bool grow_rows(int n_rows, std::string &err);
    bool grow_search(int n_rows, int nq, int k, std::string &err);
    void enqueue_queries(int nq, int kq, const int32_t *d_qids, const float *d_qw, hipStream_t s);
    void enqueue_chunk(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                       const uint32_t *d_allow);
    void drop_postings();
    bool grow_inverted(int n_rows, int nqc, int k, std::string &err);
    bool inverted_ok(std::string &err) const;
    void enqueue_chunk_inverted(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                                const uint32_t *d_allow);

    int n_vocab_ = 0, width_ = 0, dtype_ = 0;
    int cap_ = 0;                                        // capacity in rows, a multiple of 64 (the rows, n_, and the bitmap: index_frame.h)
    void *sids_ = nullptr, *sweights_ = nullptr;        // [cap_ / 64][width_][64]
    int32_t *counts_ = nullptr;                         // [cap_]
    DevBuf images_;                                     // the current chunk's query images
    DevBuf stage_;                                      // host routes: rows / queries / row ids in
    DevBuf text_in_, text_out_;                         // text routes
    DevBuf cand_in_;                                    // host routes: a caller's candidate lists
    DevBuf hyb_scores_, hyb_mask_;                      // hybrid search: the current chunk's dense scores [HC][ld]; live & live & allow
    // postings: offsets [segments][n_vocab + 1], row numbers and weights [segments][inv_seg_ * width_]; the rows they cover and the
    // segment size they were built with; the current chunk's sorted queries (ids | weights [chunk][256], then the counts)
    DevBuf poff_, prow_, pw_, qterms_;
    bool inverted_ = false;
    int inv_rows_ = 0, inv_seg_ = 0;
    int res_nq_ = 0, res_k_ = 1;                        // what reserve was last given
};

// host queries [nq][kq] as search_host checks them: every id in [-1, n_vocab), none twice in a query, every used weight finite;
// false + err names the first offender
bool sparse_queries_ok(int nq, int kq, const int32_t *qids, const float *qw, int n_vocab, std::string &err);

}  // namespace bert_hip
