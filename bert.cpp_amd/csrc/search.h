// search.h — an embedding index in HBM and its exact top-k inner-product search (the class: index.cpp; its kernels: search.hip
// behind search_kernels.h; C ABI: bert_hip_index_* in include/bert_hip.h).  Rows live on the device of the engine the index was made from, as f32, as f16 (RNE), as i8 codes with a
// scale or as one sign bit per element (b1), each row zero-padded to the k-step of the score kernel's MFMA.  A search is a GEMM (queries x rows x dim) whose epilogue selects
// instead of storing: index_topk_kernel keeps a top-k per (query, slice of rows) in LDS, topk_merge_kernel merges the
// slices' lists per query.  The score matrix never reaches HBM.
//
// Removed rows: from the first remove() on, the index keeps one bit per row (set = live) in device words and in a host mirror
// (index_frame.h; the invariant: live_bits.h).  A search then (or with an allow-list, a second bitmap of the same shape from
// the caller) runs the masked instantiation of index_topk_kernel.  An index that never saw a removal has no bitmap and
// launches what it always did.
//
// Rescoring: index_rescore_kernel scores each query against the rows its own candidate list names (the same ScoreBlock as
// the search, hence the same score bits) into [nq][n_cand] lists in the workspace, and topk_merge_kernel selects from them.
// A two-stage search is a search of a coarse index (b1, say) with k' = n_cand whose ids stay on the device and are rescored
// against a finer index of the same rows.
//
// Partition (index_partition.cpp; the list tables: partition.h): centroids, held as an f32 Index of their own, and one list id
// per row — the id a k = 1 search of that index returns for the row as get_rows gives it.  Storage stays in id order; the lists
// are a table of row ids sorted by (list, id).  A probed search scores the centroids (a search with k = nprobe), then
// index_probe_kernel scans the members of each query's lists and the unassigned tail — the rows added since — and selects on
// chip; topk_merge_kernel merges the items' lists.  kmeans refines centroids with the same assignment and kmeans_update_kernel.
// With an allow-list the scan runs index_probe_kernel's masked instantiation; a two-stage search may take the probed search as its
// coarse stage; the partition (centroids, list ids, the tail's start) has a file of its own, which a load installs as it is.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"
#include "index_file.h"
#include "index_frame.h"

namespace bert_hip {

class Index : private IndexFrame {
public:
    static constexpr int MAX_K = 256, MAX_DIM = INDEX_MAX_DIM;
    static constexpr int QCHUNK = 4096;                  // queries per internal pass (workspace bound)
    static constexpr int MAX_CAND = 1024;                // candidates per query of a rescore

    // dtype 0: f32 rows, 1: f16 rows (queries rounded to f16 as well), 2: i8 rows with one f32 scale each (queries quantized
    // the same way; search.hip), 3: one sign bit per element, no scale (queries quantized to i8 codes and a scale)
    static Index *create(Engine *eng, int dim, int dtype, std::string &err);
    ~Index();

    int size() const { return n_; }
    int n_live() const { return n_ - bits_.n_removed; }
    int dim() const { return dim_; }
    int dtype() const { return dtype_; }
    hipStream_t stream() const { return stream_; }

    // storage for n_rows rows and the workspace of searches of up to n_queries queries with any k' <= k, now
    bool reserve(int n_rows, int n_queries, int k, std::string &err);
    // append f32 rows [n][dim]: the first new id, -1 on error (index unchanged)
    int add_device(int n, const float *d_rows, hipStream_t s, std::string &err);     // asynchronous on s
    int add_host(int n, const float *rows, std::string &err);                        // blocking
    // ids / scores [nq][k], best first; 0 or -1.  d_allow: null, or device words (bit b of word w set = row 32 w + b may be
    // returned), at least ceil(size / 32) of them
    int search_device(int nq, const float *d_q, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                      const uint32_t *d_allow = nullptr);
    // host results (written only on success), queries in host (q_on_device = false) or device memory; allow: null or host
    // words as above; blocking
    int search_to_host(int nq, const float *q, bool q_on_device, int k, int32_t *ids, float *scores, std::string &err,
                       const uint32_t *allow = nullptr);
    // Rescoring: ids / scores [nq][k] = the best k of each query's own candidates d_cand [nq][n_cand] (ids; < 0, >= size and
    // removed rows are skipped; repeats count as often as they appear), scored as a search scores them.  1 <= n_cand <=
    // MAX_CAND, 1 <= k <= MAX_K.  Asynchronous on s; 0 or -1
    int rescore_device(int nq, const float *d_q, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids, float *d_scores,
                       hipStream_t s, std::string &err);
    // host queries, candidates (every id in [-1, size): the caller checks) and results (written only on success); blocking
    int rescore_to_host(int nq, const float *q, int n_cand, const int32_t *cand, int k, int32_t *ids, float *scores, std::string &err);
    // Two-stage search: coarse.search_device with k' = n_cand, the ids kept on the device, then this index's rescore_device
    // with the same f32 queries.  The caller checks that both live on one engine and have equal dim and size, and
    // 1 <= k <= n_cand <= MAX_K.  Asynchronous on s; 0 or -1.  nprobe > 0: the coarse stage is coarse.search_probed_device with
    // that nprobe and the allow-list (device / host words covering coarse, or null), under that call's conditions
    int search_rescored_device(Index &coarse, int nq, const float *d_q, int n_cand, int k, int32_t *d_ids, float *d_scores,
                               hipStream_t s, std::string &err, int nprobe = 0, const uint32_t *d_allow = nullptr);
    int search_rescored_to_host(Index &coarse, int nq, const float *q, int n_cand, int k, int32_t *ids, float *scores, std::string &err,
                                int nprobe = 0, const uint32_t *allow = nullptr);
    // the stored rows ids [n] (each in [0, size): the caller checks) as f32 [n][dim], removed rows included; blocking
    int get_rows(int n, const int32_t *ids, float *rows, std::string &err);
    // Partition.  partition: installs centroids [n_lists][dim] (finite: the caller checks; 1 <= n_lists <= MAX_LISTS) and
    // assigns every current row; n_lists = 0 drops the partition.  Rows added later are the unassigned tail.  Blocking; 0 or -1
    static constexpr int MAX_LISTS = 65536;
    int partition(int n_lists, const float *centroids, std::string &err);
    int n_lists() const { return cent_ ? cent_->size() : 0; }
    const std::vector<float> &centroids() const { return cent_h_; }
    void partition_lists(int32_t *list_of_row) const;               // [size]: -1 for the tail
    // spherical k-means over the live rows: n_iter times assign as partition does, then each centroid := its members' sum
    // over that sum's norm (kept for no member, a zero or a non-finite norm).  Leaves the index as it is.  Blocking; 0 or -1
    int kmeans(int n_lists, int n_iter, float *centroids, std::string &err);
    // Probed search: as search_device over the rows of each query's nprobe best lists and the tail.  The caller checks that
    // there is a partition and 1 <= nprobe <= min(n_lists, MAX_K).  Asynchronous on s; 0 or -1.  d_allow / allow: as search_device's
    // and search_to_host's — with one, index_probe_kernel's masked instantiation over the same items and workspace
    int search_probed_device(int nq, const float *d_q, int nprobe, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                             const uint32_t *d_allow = nullptr);
    int search_probed_to_host(int nq, const float *q, int nprobe, int k, int32_t *ids, float *scores, std::string &err,
                              const uint32_t *allow = nullptr);
    // The partition as a file of its own (index_file.h; the format is stated in include/bert_hip.h).  save_partition: the caller
    // checks that there is one.  load_partition installs the file's centroids and lists as they are — no assignment runs, the
    // rows at and beyond its n_part are the tail —: 0, -2 (the file does not fit the index, or holds a non-finite centroid or a
    // list id outside the lists) or -3, the index keeping the partition it had.  Blocking
    bool save_partition(const char *path, std::string &err);
    int load_partition(const char *path, std::string &err);
    // marks rows as removed (ids in [0, size) or -1 with the index unchanged; repeats ignored): the number newly removed; blocking
    int remove(int n, const int32_t *ids, std::string &err);
    // drops the removed rows' storage: live rows keep order and bits, ids 0 .. n_live - 1; old_ids (null or [n_live]) the
    // former ids; the new size or -1; blocking
    int compact(int32_t *old_ids, std::string &err);
    // the index as stored to / from a file (index_file.h); load_rows: into an empty index made for the header's dim and dtype,
    // f positioned behind the header
    bool save(const char *path, std::string &err);
    bool load_rows(FILE *f, const IndexFileHeader &h, std::string &err);
    // a device f32 buffer of at least n floats for the text routes (the index's operations that read it are finished)
    float *scratch(size_t n, std::string &err);
    // forget the rows behind the first n (an add of several parts that failed part way)
    void truncate(int n);

private:
    friend struct Hybrid;                               // hybrid.h: a search over this index and a sparse index together
    Index() = default;
    bool grow_rows(int n_rows, std::string &err);
    void enqueue_chunk(int nq, const float *d_q, int k, int32_t *d_ids, float *d_scores, hipStream_t s, const uint32_t *d_allow);
    void enqueue_queries(int nq, const float *d_q, hipStream_t s);
    int host_route(int nq, const float *q, bool q_on_device, bool wait, int k, int32_t *ids, float *scores, std::string &err,
                   const std::function<int(int, int, const float *, int32_t *, float *)> &device_form);
    bool grow_queries(int nqc, std::string &err);
    void enqueue_export(int first, int n, const int32_t *d_ids, float *d_out, hipStream_t s);
    bool assign_rows(Index &cent, std::vector<int32_t> &list_of, std::string &err);
    bool upload_lists(const std::vector<int32_t> &list_of, int n_lists, std::string &err);
    bool install_partition(std::unique_ptr<Index> cent, const float *centroids, std::vector<int32_t> &&list_of, std::string &err);
    void drop_partition();

    int dim_ = 0, dtype_ = 0, dpad_ = 0;                // dpad_: elements per stored row
    size_t row_bytes_ = 0, qrow_bytes_ = 0;             // bytes per stored row; per query as the score kernel reads it (b1: i8 codes)
    int cap_ = 0;                                       // (the rows themselves, n_, the bitmap, the lists' workspace: index_frame.h)
    void *rows_ = nullptr;                              // [cap_][row_bytes_]
    float *rscale_ = nullptr;                           // i8: [cap_] row scales
    DevBuf qbuf_;                                       // the current chunk's queries as stored
    DevBuf qscale_;                                     // i8, b1: the current chunk's query scales
    DevBuf cand_i_, cand_s_, cand_in_;                  // two-stage search: the coarse stage's lists; host rescore: the caller's ids
    // partition: the centroids as an index (null: none) and on the host; the list of each row below n_part_ (the rows behind
    // are the tail); the list tables on the device; the probed lists of the current chunk; exported rows and their lists
    std::unique_ptr<Index> cent_;
    std::vector<float> cent_h_;
    std::vector<int32_t> list_of_;
    int n_part_ = 0;
    DevBuf offsets_, order_, probe_i_, probe_s_, export_, assign_i_, assign_s_;
    DevBuf stage_, scratch_;                            // host routes: f32 rows / queries; the text routes' embeddings
};

// How a search cuts a chunk of nq queries with this k over n_rows rows into workgroups of index_topk_kernel — what plan() of
// index.cpp gives enqueue_chunk —: geometry = {query tiles, slices, rows per slice, entries of a query's LDS list}.  For the test
// hook bert_hip_test_index_plan; no device.
void index_search_plan(int n_rows, int nq, int k, int geometry[4]);

}  // namespace bert_hip
