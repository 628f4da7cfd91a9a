// token_index.h — a token index in HBM and its exact MaxSim top-k search (the class: token_index.cpp; its kernels: token_index.hip
// behind token_index_kernels.h; C ABI: bert_hip_token_index_* in include/bert_hip.h).  Documents are runs of f16 token rows, packed,
// with int32 cumulative lengths on the device and in a host mirror, on the device of the engine the index was made from.  A search
// scans the documents with one (query, slice of documents) per workgroup and selects on chip (token_index_scan_kernel), then merges the
// slices' lists per query with the embedding index's topk_merge_kernel; a rescore turns per-query candidate ids into maxsim's pair
// list, scores them with launch_maxsim against the index's own arrays and selects with the same merge.  Grow-only storage and
// workspace; the event, the stream of the host routes and the removed-documents bitmap are the frame's that all three indexes derive
// from (index_frame.h; the bitmap's invariant: live_bits.h).  The bitmap is there from the first remove to the next compact; while it exists, or under
// an allow-list, a search launches the masked scan and a rescore's pair list leaves the removed ids out.  compact gathers the live
// documents' rows into a fresh allocation on the device; save / load move the file form (token_index_file.h) in pieces.
// dtype 2, the int8 form (token_index_kernels.h states it): rows are int8 codes of dpad bytes with one f32 scale per token, every add
// quantises on the device, a search quantises its queries into a workspace that reserve sizes and scans with token_index_scan_kernel's
// int8 form, and a rescore is the same kernel over the candidate lists instead of maxsim.  The bitmap, the event, the streams, the
// chunk loop, commit and the host mirrors are the f16 form's.  compact, save and load are the f16 form's alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "engine.h"
#include "index_frame.h"
#include "token_index_file.h"
#include "token_index_kernels.h"

namespace bert_hip {

class TokenIndex : private IndexFrame {
public:
    static constexpr int MAX_K = 256, MAX_CAND = TOKEN_MAX_CAND;
    static constexpr int QCHUNK = 256;                   // queries per internal pass (workspace bound)

    static TokenIndex *create(Engine *eng, int dim, std::string &err) { return create(eng, dim, 1, err); }
    // dtype: 1 = f16 rows, 2 = int8 codes with per-token scales
    static TokenIndex *create(Engine *eng, int dim, int dtype, std::string &err);
    ~TokenIndex();

    int size() const { return n_; }
    int64_t n_tokens() const { return n_tok_; }
    int n_live() const { return n_ - bits_.n_removed; }
    int64_t n_live_tokens() const { return n_tok_ - tok_removed_; }
    int dim() const { return dim_; }
    int dtype() const { return dtype_; }
    int dpad() const { return dpad_; }                   // int8 form: the bytes of a stored row
    // (the int8 form: 128 at every dim, and the limit of a rescore's queries too)
    int max_query_tokens() const { return token_max_query_tokens(dim_, dtype_); }
    hipStream_t stream() const { return stream_; }

    // Results: >= 0, or -2 (an argument the entry refuses; nothing changed) or -3 (a device error), a message in err either way.
    // storage for n_docs documents of n_tokens tokens in all, and the workspace of searches of up to n_queries queries of up to
    // max_q_len tokens with any k' <= k, now
    int reserve(int n_docs, int64_t n_tokens, int n_queries, int max_q_len, int k, std::string &err);
    // append n_docs documents: cu [n_docs + 1] in HOST memory (checked), d_rows f16 in device memory indexed by cu: the first new id.
    // Asynchronous on s; may grow storage (not for stream capture)
    int add_device(int n_docs, const int32_t *cu, const half_t *d_rows, hipStream_t s, std::string &err);
    // host rows f32 indexed by cu, rounded to f16 on the device; blocking
    int add_host(int n_docs, const int32_t *cu, const float *rows, std::string &err);
    // Text route: room for n_tokens more rows (storage grown, the index's operations that read the old storage finished), the place the
    // next document's first row goes — the caller writes the rows there on stream() and commits them with add_in_place.  The int8 form
    // hands out a buffer of its own for the f16 rows, and add_in_place quantises them from there into storage
    half_t *append_room(int64_t n_tokens, std::string &err);
    // the n_docs documents whose rows the caller has enqueued on stream() at append_room's place; cu relative (cu[0] == 0), checked
    int add_in_place(int n_docs, const int32_t *cu, std::string &err);
    // forget the documents behind the first n (an add of several parts that failed part way)
    void truncate(int n);
    // document id's rows as f32 [len][dim] (the stored f16 values converted exactly): its length; writes iff cap_tokens >= it.  Blocking
    // (the int8 form: (float)code * scale)
    int get_doc(int id, float *rows, int cap_tokens, std::string &err);
    // int8 form: the document's codes [len][dpad] and scales [len] as stored: its length; writes iff cap_tokens >= it.  f16 form: -2
    int get_codes(int id, int8_t *codes, float *scales, int cap_tokens, std::string &err);
    // ids / scores [nq][k], best first; queries d_q f16 indexed by d_qcu [nq + 1], both in device memory, unchecked (the kernel's
    // guards).  max_q_len: the caller's promise, 1 .. max_query_tokens().  Asynchronous on s.  d_allow: null, or device words
    // [ceil(size / 32)], bit set = the document may be returned
    int search_device(int nq, const int32_t *d_qcu, const half_t *d_q, int max_q_len, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                      std::string &err, const uint32_t *d_allow = nullptr);
    // host queries (qcu strictly ascending from an entry >= 0, no query longer than max_query_tokens(); rows f32, rounded to f16 on the
    // device) and host results (written only on success); blocking.  allow: null, or host words as d_allow
    int search_host(int nq, const int32_t *qcu, const float *q_rows, int k, int32_t *ids, float *scores, std::string &err,
                    const uint32_t *allow = nullptr);
    // a device search on stream() and its results -> host; blocking
    int search_device_to_host(int nq, const int32_t *d_qcu, const half_t *d_q, int max_q_len, int k, int32_t *ids, float *scores, std::string &err,
                              const uint32_t *d_allow = nullptr) {
        return search_to_host(nq, d_qcu, d_q, false, max_q_len, k, ids, scores, err, d_allow);
    }
    // Per query its n_cand candidates d_cand [nq][n_cand] (ids outside [0, size) and removed documents: no candidate) scored with the search's bits, the best
    // k to d_ids / d_scores [nq][k].  The workspace grows on demand and is not part of reserve.  Asynchronous on s.  (The int8 form
    // stages a query as the search does: one of more than max_query_tokens() tokens gets -1 / -INFINITY)
    int rescore_device(int nq, const int32_t *d_qcu, const half_t *d_q, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids, float *d_scores,
                       hipStream_t s, std::string &err);
    // host queries (checked as search_host's, of any length — int8 form: at most max_query_tokens()), candidates (each in [-1, size), -2
    // otherwise) and results; blocking
    int rescore_host(int nq, const int32_t *qcu, const float *q_rows, int n_cand, const int32_t *cand, int k, int32_t *ids, float *scores,
                     std::string &err);
    // Text routes: device buffers of the index for a chunk's packed token ids | cu_seqlens (in) and, for queries, its f16 rows (out)
    bool text_buffers(size_t in_bytes, size_t out_bytes, char *&d_in, char *&d_out, std::string &err);
    // Removed documents: the number newly removed (repeats and removed documents are ignored); an id outside [0, size): -2, nothing
    // changed.  The first one allocates the bitmap.  Blocking
    int remove(int n, const int32_t *ids, std::string &err);
    // Drops the removed documents: the live ones keep their order and bits and get ids 0 .. n_live - 1; old_ids (nullable) [n_live]
    // receives their former ids.  The new size; the bitmap is gone afterwards.  Fresh storage for the live rows beside the old (the
    // peak is old + new); -3 and the index unchanged where that fails.  Blocking.  The int8 form: -2, the index unchanged
    int compact(int32_t *old_ids, std::string &err);
    // the file form (token_index_file.h), rows in pieces of 32 MiB through a host buffer; blocking.  load: from f, positioned behind
    // the header h that token_index_header_check passed
    // (f16 form only: the C ABI refuses an int8 index with -2 in front of this)
    bool save(const char *path, std::string &err);
    static TokenIndex *load(Engine *eng, FILE *f, const TokenIndexFileHeader &h, std::string &err);

private:
    TokenIndex() = default;
    bool grow_storage(long long n_docs, long long n_tokens, std::string &err);
    bool grow_search(int n_docs, int nqc, int k, std::string &err);
    // int8 form: the queries' codes and scales, [nqc][max_q_len] rows
    bool grow_queries(int nqc, int max_q_len, std::string &err);
    size_t row_bytes() const { return dtype_ == 2 ? (size_t)dpad_ : (size_t)dim_ * 2; }
    // int8 form: n rows (f32 or f16, device memory) -> codes and scales from stored row `at` on, on s
    void quantize_rows(const void *d_src, bool src_f32, long long n, long long at, hipStream_t s);
    // the searches and rescores behind the public forms: the queries d_q are f16, or (q_f32: the host forms of the int8 index) f32
    int search_any(int nq, const int32_t *d_qcu, const void *d_q, bool q_f32, int max_q_len, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                   std::string &err, const uint32_t *d_allow);
    int search_to_host(int nq, const int32_t *d_qcu, const void *d_q, bool q_f32, int max_q_len, int k, int32_t *ids, float *scores, std::string &err,
                       const uint32_t *d_allow);
    // the chunk loop behind every search (d_cand null: the documents under live_ / d_allow) and the int8 rescore (d_cand [nq][n_cand])
    int scan_chunks(int nq, const int32_t *d_qcu, const void *d_q, bool q_f32, int max_q_len, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                    std::string &err, const uint32_t *d_allow, const int32_t *d_cand, int n_cand);
    // out_ids_ / out_scores_ [nq][k] -> the caller's arrays behind what stream() holds; blocking
    int deliver_results(const char *what, int nq, int k, int32_t *ids, float *scores, std::string &err);
    // cu entries of n_docs new documents (lengths from cu, any base) behind the stored ones, on s; bumps the counts
    bool commit(int n_docs, const int32_t *cu, hipStream_t s, std::string &err);
    // queries of a host form: rows -> f16 in q16_ (the int8 form: left as f32 in stage_), lengths (rebased to 0) -> qcu_in_, on
    // stream(); max_len: the longest
    int stage_queries(const char *what, int nq, const int32_t *qcu, const float *q_rows, int limit, int &max_len, std::string &err);

    int dim_ = 0, dtype_ = 1, dpad_ = 0;
    int cap_docs_ = 0;                                  // capacity of cu_ in documents (the documents, n_, and the bitmap: index_frame.h)
    int64_t n_tok_ = 0, cap_tok_ = 0;                   // rows; capacity of rows_ in rows
    char *rows_ = nullptr;                              // [cap_tok_][row_bytes()]: f16 rows, or int8 codes
    float *scales_ = nullptr;                           // int8 form: [cap_tok_]
    int32_t *cu_ = nullptr;                             // [cap_docs_ + 1]
    std::vector<int32_t> cu_h_;                         // the host mirror, [n_ + 1]
    int64_t tok_removed_ = 0;                           // the removed documents' rows (0 without a bitmap)
    std::vector<int32_t> qcu_h_;                        // host routes: the current call's query lengths, rebased to 0
    DevBuf pairs_;                                      // a rescore's pair list
    DevBuf stage_, q16_, qcu_in_, cand_in_;             // host routes: f32 rows in, queries, candidates
    DevBuf text_in_, text_out_;                         // text routes
    DevBuf text_rows_;                                  // int8 form: the f16 rows of an add_texts chunk (append_room)
    DevBuf q_codes_, q_scales_;                         // int8 form: the quantised queries of a search or rescore
};

// cu [n + 1] ascends strictly from an entry >= 0 (no empty entry)
bool token_cu_ok(const int32_t *cu, int n);

}  // namespace bert_hip
