// hybrid_api.cpp — the entry points of bert_hip.h that search an embedding index and a sparse index together (hybrid.h): the
// bert_hip_hybrid_* ones, which scan the sparse index's rows, and the bert_hip_dense_sparse_search_inverted* ones, which walk its
// postings and return the same ids and score bits.  Each pair shares one body.  The text route encodes with the dense index's context
// into that index's scratch buffer, runs the MLM head of the sparse index's context into that index's text buffers, and hands both to
// the device form on the sparse index's stream: neither the embeddings nor the terms reach the host.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bert_hip.h"
#include "abi.h"
#include "hybrid.h"
#include "text_routes.h"

using namespace bert_hip;

namespace {

// The frame of an entry point that takes both indexes: -1 (after a line on stderr) without one of them, else the body's result; a body
// that returns -2 or -3 has put its message into err, and it is printed here.  -4 for an exception.
template <class F>
int32_t hybrid_call(const char *me, bert_hip_index *dense, bert_hip_sparse_index *sparse, F &&body) {
    return guarded(me, [&]() -> int32_t {
        if (!dense || !dense->ix) { fprintf(stderr, "%s: no embedding index\n", me); return -1; }
        if (!sparse || !sparse->ix) { fprintf(stderr, "%s: no sparse index\n", me); return -1; }
        std::string err;
        const int32_t r = body(*dense->ix, *sparse->ix, err);
        if ((r == -2 || r == -3) && !err.empty()) fprintf(stderr, "%s: %s\n", me, err.c_str());
        return r;
    }, (int32_t)-4);
}

// the three forms, over the rows or (inverted) over the postings
int32_t search_host_entry(const char *me, bool inverted, bert_hip_index *dense, bert_hip_sparse_index *sparse, int32_t n_queries, const float *queries,
                          int32_t kq, const int32_t *q_ids, const float *q_weights, float w_dense, float w_sparse, const uint32_t *allow,
                          int32_t n_words, int32_t k, int32_t *ids, float *scores) {
    return hybrid_call(me, dense, sparse, [&](Index &d, SparseIndex &sp, std::string &err) -> int32_t {
        if (const int go = Hybrid::check(d, sp, n_queries, queries && q_ids && q_weights && ids && scores, kq, w_dense, w_sparse, allow, n_words, k, err, inverted); go <= 0) return go;
        return Hybrid::search_host(d, sp, n_queries, queries, kq, q_ids, q_weights, w_dense, w_sparse, allow, k, ids, scores, err, inverted);
    });
}

int32_t search_device_entry(const char *me, bool inverted, bert_hip_index *dense, bert_hip_sparse_index *sparse, int32_t n_queries,
                            const float *d_queries, int32_t kq, const int32_t *d_q_ids, const float *d_q_weights, float w_dense, float w_sparse,
                            const uint32_t *d_allow, int32_t n_words, int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    return hybrid_call(me, dense, sparse, [&](Index &d, SparseIndex &sp, std::string &err) -> int32_t {
        if (const int go = Hybrid::check(d, sp, n_queries, d_queries && d_q_ids && d_q_weights && d_ids && d_scores, kq, w_dense, w_sparse, d_allow, n_words, k, err, inverted); go <= 0) return go;
        return Hybrid::search_device(d, sp, n_queries, d_queries, kq, d_q_ids, d_q_weights, w_dense, w_sparse, d_allow, k, d_ids, d_scores, (hipStream_t)stream, err, inverted);
    });
}

int32_t search_texts_entry(const char *me, bool inverted, bert_hip_index *dense, bert_hip_sparse_index *sparse, int32_t n_threads, int32_t n_queries,
                           const char **texts, int32_t kq, float w_dense, float w_sparse, int32_t k, int32_t *ids, float *scores) {
    return hybrid_call(me, dense, sparse, [&](Index &d, SparseIndex &sp, std::string &err) -> int32_t {
        bert_ctx *dctx = dense->ctx, *sctx = sparse->ctx;
        if (d.dim() != dctx->hp.n_embd) { err = "the embedding index has dim " + std::to_string(d.dim()) + ", its model's embeddings " + std::to_string(dctx->hp.n_embd); return -2; }
        if (!text_model_ok(sctx, sp, err)) return -2;
        if (const int go = Hybrid::check(d, sp, n_queries, texts && ids && scores, kq, w_dense, w_sparse, nullptr, 0, k, err, inverted); go <= 0) return go;
        // (the outputs are written only when every chunk has succeeded)
        std::vector<int32_t> hid((size_t)n_queries * k);
        std::vector<float> hsc((size_t)n_queries * k);
        const int32_t H = dctx->hp.n_embd, GROUP = 4096;             // (the sparse route's groups: a group's embeddings, then its chunks of terms)
        std::vector<float> emb;
        for (int32_t i0 = 0; i0 < n_queries; i0 += GROUP) {
            const int32_t m = std::min(GROUP, n_queries - i0);
            const float *d_emb = nullptr;
            if (dctx->engines.size() > 1) {
                // (a context over several GPUs encodes through the host, as bert_hip_index_search_texts does there)
                float *buf = encode_host(dctx, n_threads, m, texts + i0, emb, err) ? d.scratch((size_t)m * H, err) : nullptr;
                if (!buf || hipMemcpy(buf, emb.data(), (size_t)m * H * 4, hipMemcpyHostToDevice) != hipSuccess) { if (err.empty()) err = "device error"; return -3; }
                d_emb = buf;
            } else if (!encode_groups_device(dctx, d, n_threads, m, texts + i0, [&](int32_t, int32_t, const float *rows) { d_emb = rows; return true; }, err)) {
                if (err.empty()) err = "device error";
                return -3;
            }
            const int32_t r = sparse_text_chunks(sctx, sp, n_threads, m, texts + i0, kq, [&](int32_t j0, int32_t nb, const int32_t *d_ids, const float *d_w) -> int32_t {
                return Hybrid::search_device_to_host(d, sp, nb, d_emb + (size_t)j0 * H, kq, d_ids, d_w, w_dense, w_sparse, k, hid.data() + (size_t)(i0 + j0) * k,
                                                     hsc.data() + (size_t)(i0 + j0) * k, err, inverted);
            }, err);
            if (r != 0) { if (err.empty()) err = "device error"; return r; }
        }
        memcpy(ids, hid.data(), hid.size() * 4);
        memcpy(scores, hsc.data(), hsc.size() * 4);
        return 0;
    });
}

}  // namespace

extern "C" {

int32_t bert_hip_hybrid_reserve(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_rows, int32_t n_queries, int32_t k) {
    return hybrid_call("bert_hip_hybrid_reserve", dense, sparse, [&](Index &d, SparseIndex &sp, std::string &err) {
        return Hybrid::reserve(d, sp, n_rows, n_queries, k, err);
    });
}

int32_t bert_hip_hybrid_search(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries, const float *queries,
                               int32_t kq, const int32_t *q_ids, const float *q_weights, float w_dense, float w_sparse, const uint32_t *allow,
                               int32_t n_words, int32_t k, int32_t *ids, float *scores) {
    return search_host_entry("bert_hip_hybrid_search", false, dense, sparse, n_queries, queries, kq, q_ids, q_weights, w_dense, w_sparse, allow, n_words, k, ids, scores);
}

int32_t bert_hip_hybrid_search_device(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries, const float *d_queries,
                                      int32_t kq, const int32_t *d_q_ids, const float *d_q_weights, float w_dense, float w_sparse,
                                      const uint32_t *d_allow, int32_t n_words, int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    return search_device_entry("bert_hip_hybrid_search_device", false, dense, sparse, n_queries, d_queries, kq, d_q_ids, d_q_weights, w_dense, w_sparse, d_allow,
                               n_words, k, d_ids, d_scores, stream);
}

int32_t bert_hip_hybrid_search_texts(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_threads, int32_t n_queries,
                                     const char **texts, int32_t kq, float w_dense, float w_sparse, int32_t k, int32_t *ids, float *scores) {
    return search_texts_entry("bert_hip_hybrid_search_texts", false, dense, sparse, n_threads, n_queries, texts, kq, w_dense, w_sparse, k, ids, scores);
}

int32_t bert_hip_dense_sparse_search_inverted(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries, const float *queries,
                                              int32_t kq, const int32_t *q_ids, const float *q_weights, float w_dense, float w_sparse,
                                              const uint32_t *allow, int32_t n_words, int32_t k, int32_t *ids, float *scores) {
    return search_host_entry("bert_hip_dense_sparse_search_inverted", true, dense, sparse, n_queries, queries, kq, q_ids, q_weights, w_dense, w_sparse, allow, n_words,
                             k, ids, scores);
}

int32_t bert_hip_dense_sparse_search_inverted_device(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries,
                                                     const float *d_queries, int32_t kq, const int32_t *d_q_ids, const float *d_q_weights,
                                                     float w_dense, float w_sparse, const uint32_t *d_allow, int32_t n_words, int32_t k,
                                                     int32_t *d_ids, float *d_scores, void *stream) {
    return search_device_entry("bert_hip_dense_sparse_search_inverted_device", true, dense, sparse, n_queries, d_queries, kq, d_q_ids, d_q_weights, w_dense, w_sparse,
                               d_allow, n_words, k, d_ids, d_scores, stream);
}

int32_t bert_hip_dense_sparse_search_inverted_texts(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_threads,
                                                    int32_t n_queries, const char **texts, int32_t kq, float w_dense, float w_sparse, int32_t k,
                                                    int32_t *ids, float *scores) {
    return search_texts_entry("bert_hip_dense_sparse_search_inverted_texts", true, dense, sparse, n_threads, n_queries, texts, kq, w_dense, w_sparse, k, ids, scores);
}

}  // extern "C"
