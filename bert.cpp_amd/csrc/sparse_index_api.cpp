// sparse_index_api.cpp — the bert_hip_sparse_index_* entry points of bert_hip.h: a sparse index (sparse_index.h) on a context's first
// device.  The text routes tokenize and pack as bert_hip_encode_sparse_batch does, run the MLM head's top-k form into the index's device
// buffers and hand those to add_device / search_device: the terms never reach the host.  remove, the filtered searches, rescore,
// compact and save are frames around the class; load checks the file's header (sparse_index_file.h) before it makes the index.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../../include/bert_hip.h"
#include "abi.h"
#include "sparse_index_file.h"
#include "text_routes.h"

using namespace bert_hip;

namespace {

// The frame of an entry point that takes a sparse index: -1 (after a line on stderr) without one, else the body's result; a body
// that returns -2 or -3 has put its message into err, and it is printed here.  -4 for an exception.
template <class F>
int32_t sparse_index_call(const char *me, bert_hip_sparse_index *ix, F &&body) {
    return guarded(me, [&]() -> int32_t {
        if (!ix || !ix->ix) { fprintf(stderr, "%s: no index\n", me); return -1; }
        std::string err;
        const int32_t r = body(ix->ctx, *ix->ix, err);
        if ((r == -2 || r == -3) && !err.empty()) fprintf(stderr, "%s: %s\n", me, err.c_str());
        return r;
    }, (int32_t)-4);
}

// an allow-list of n_words words covers the index (-2 + err otherwise)
bool allow_ok(const SparseIndex &x, const uint32_t *allow, int32_t n_words, std::string &err) {
    const int64_t need = ((int64_t)x.size() + 31) / 32;
    if (!allow || n_words >= need) return true;
    err = "the allow-list has " + std::to_string(n_words) + " words, an index of " + std::to_string(x.size()) + " rows needs " + std::to_string(need);
    return false;
}

// (the text routes' way from texts to the index's device buffers, text_model_ok and sparse_text_chunks: text_routes.h)

}  // namespace

extern "C" {

struct bert_hip_sparse_index *bert_hip_sparse_index_create(struct bert_ctx *ctx, int32_t n_vocab, int32_t width, int32_t dtype) {
    return guarded("bert_hip_sparse_index_create", [&]() -> bert_hip_sparse_index * {
        const char *me = "bert_hip_sparse_index_create";
        if (!ctx) { fprintf(stderr, "%s: no context\n", me); return nullptr; }
        if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device (tokenizer-only): an index lives on the context's device\n", me); return nullptr; }
        if (n_vocab == 0) n_vocab = ctx->hp.n_vocab;
        std::string err;
        std::unique_ptr<SparseIndex> ix(SparseIndex::create(ctx->engine(), n_vocab, width, dtype, err));
        if (!ix) { fprintf(stderr, "%s: %s\n", me, err.c_str()); return nullptr; }
        std::unique_ptr<bert_hip_sparse_index> h(new bert_hip_sparse_index);
        h->ctx = ctx;
        h->ix = std::move(ix);
        ctx->sparse_indexes.push_back(h.get());
        return h.release();
    }, (bert_hip_sparse_index *)nullptr);
}

void bert_hip_sparse_index_free(struct bert_hip_sparse_index *ix) {
    guarded("bert_hip_sparse_index_free", [&] {
        if (!ix) return;
        auto &v = ix->ctx->sparse_indexes;
        v.erase(std::remove(v.begin(), v.end(), ix), v.end());
        delete ix;
    });
}

int32_t bert_hip_sparse_index_size(struct bert_hip_sparse_index *ix) { return ix && ix->ix ? ix->ix->size() : -1; }

int32_t bert_hip_sparse_index_reserve(struct bert_hip_sparse_index *ix, int32_t n_rows, int32_t n_queries, int32_t k) {
    return sparse_index_call("bert_hip_sparse_index_reserve", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) { return x.reserve(n_rows, n_queries, k, err); });
}

int32_t bert_hip_sparse_index_add(struct bert_hip_sparse_index *ix, int32_t n, int32_t k_in, const int32_t *ids, const float *weights) {
    return sparse_index_call("bert_hip_sparse_index_add", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) { return x.add_host(n, k_in, ids, weights, err); });
}

int32_t bert_hip_sparse_index_add_device(struct bert_hip_sparse_index *ix, int32_t n, int32_t k_in, const int32_t *d_ids, const float *d_weights,
                                         void *stream) {
    return sparse_index_call("bert_hip_sparse_index_add_device", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) {
        return x.add_device(n, k_in, d_ids, d_weights, (hipStream_t)stream, err);
    });
}

int32_t bert_hip_sparse_index_add_texts(struct bert_hip_sparse_index *ix, int32_t n_threads, int32_t n, const char **texts) {
    const char *me = "bert_hip_sparse_index_add_texts";
    return sparse_index_call(me, ix, [&](bert_ctx *ctx, SparseIndex &x, std::string &err) -> int32_t {
        if (!text_model_ok(ctx, x, err)) return -2;
        if (n < 0 || (n > 0 && !texts)) { err = "n >= 0 and texts required"; return -2; }
        const int first = x.size();
        if (n == 0) return first;
        const int32_t r = sparse_text_chunks(ctx, x, n_threads, n, texts, x.width(), [&](int32_t, int32_t nb, const int32_t *d_ids, const float *d_w) -> int32_t {
            const int32_t a = x.add_device(nb, x.width(), d_ids, d_w, x.stream(), err);
            return a < 0 ? a : 0;
        }, err);
        if (r == 0) return first;
        x.truncate(first);
        if (err.empty()) err = "device error";
        return r;
    });
}

int32_t bert_hip_sparse_index_search(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids, const float *q_weights,
                                     int32_t k, int32_t *ids, float *scores) {
    return sparse_index_call("bert_hip_sparse_index_search", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) {
        return x.search_host(n_queries, kq, q_ids, q_weights, k, ids, scores, err);
    });
}

int32_t bert_hip_sparse_index_search_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *d_q_ids,
                                            const float *d_q_weights, int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    return sparse_index_call("bert_hip_sparse_index_search_device", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) {
        return x.search_device(n_queries, kq, d_q_ids, d_q_weights, k, d_ids, d_scores, (hipStream_t)stream, err);
    });
}

int32_t bert_hip_sparse_index_search_texts(struct bert_hip_sparse_index *ix, int32_t n_threads, int32_t n_queries, const char **texts, int32_t kq,
                                           int32_t k, int32_t *ids, float *scores) {
    const char *me = "bert_hip_sparse_index_search_texts";
    return sparse_index_call(me, ix, [&](bert_ctx *ctx, SparseIndex &x, std::string &err) -> int32_t {
        if (!text_model_ok(ctx, x, err)) return -2;
        if (k < 1 || k > SparseIndex::MAX_K || kq < 1 || kq > SparseIndex::MAX_TERMS) { err = "1 <= k <= 256 and 1 <= kq <= 256 required"; return -2; }
        if (n_queries < 0 || (n_queries > 0 && (!texts || !ids || !scores))) { err = "n_queries >= 0 and texts / outputs required"; return -2; }
        if (n_queries == 0) return 0;
        // (the outputs are written only when every chunk has succeeded)
        std::vector<int32_t> hid((size_t)n_queries * k);
        std::vector<float> hsc((size_t)n_queries * k);
        const int32_t r = sparse_text_chunks(ctx, x, n_threads, n_queries, texts, kq, [&](int32_t i0, int32_t nb, const int32_t *d_ids, const float *d_w) -> int32_t {
            return x.search_device_to_host(nb, kq, d_ids, d_w, k, hid.data() + (size_t)i0 * k, hsc.data() + (size_t)i0 * k, err);
        }, err);
        if (r != 0) { if (err.empty()) err = "device error"; return r; }
        memcpy(ids, hid.data(), hid.size() * 4);
        memcpy(scores, hsc.data(), hsc.size() * 4);
        return 0;
    });
}

int32_t bert_hip_sparse_index_search_filtered(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids, const float *q_weights,
                                              int32_t k, const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores) {
    return sparse_index_call("bert_hip_sparse_index_search_filtered", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) -> int32_t {
        if (!allow_ok(x, allow, n_words, err)) return -2;
        return x.search_host(n_queries, kq, q_ids, q_weights, k, ids, scores, err, allow);
    });
}

int32_t bert_hip_sparse_index_search_filtered_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *d_q_ids,
                                                     const float *d_q_weights, int32_t k, const uint32_t *d_allow, int32_t n_words, int32_t *d_ids,
                                                     float *d_scores, void *stream) {
    return sparse_index_call("bert_hip_sparse_index_search_filtered_device", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) -> int32_t {
        if (!allow_ok(x, d_allow, n_words, err)) return -2;
        return x.search_device(n_queries, kq, d_q_ids, d_q_weights, k, d_ids, d_scores, (hipStream_t)stream, err, d_allow);
    });
}

// Postings and the inverted search: the frames of search_filtered[_device] and search_texts around the class's inverted form
int32_t bert_hip_sparse_index_invert(struct bert_hip_sparse_index *ix) {
    return sparse_index_call("bert_hip_sparse_index_invert", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) { return x.invert(err); });
}

int32_t bert_hip_sparse_index_inverted_rows(struct bert_hip_sparse_index *ix) { return ix && ix->ix ? ix->ix->inverted_rows() : -1; }

int32_t bert_hip_sparse_index_search_inverted(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids, const float *q_weights,
                                              int32_t k, const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores) {
    return sparse_index_call("bert_hip_sparse_index_search_inverted", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) -> int32_t {
        if (!allow_ok(x, allow, n_words, err)) return -2;
        return x.search_host(n_queries, kq, q_ids, q_weights, k, ids, scores, err, allow, true);
    });
}

int32_t bert_hip_sparse_index_search_inverted_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *d_q_ids,
                                                     const float *d_q_weights, int32_t k, const uint32_t *d_allow, int32_t n_words, int32_t *d_ids,
                                                     float *d_scores, void *stream) {
    return sparse_index_call("bert_hip_sparse_index_search_inverted_device", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) -> int32_t {
        if (!allow_ok(x, d_allow, n_words, err)) return -2;
        return x.search_device(n_queries, kq, d_q_ids, d_q_weights, k, d_ids, d_scores, (hipStream_t)stream, err, d_allow, true);
    });
}

int32_t bert_hip_sparse_index_search_inverted_texts(struct bert_hip_sparse_index *ix, int32_t n_threads, int32_t n_queries, const char **texts, int32_t kq,
                                                    int32_t k, int32_t *ids, float *scores) {
    const char *me = "bert_hip_sparse_index_search_inverted_texts";
    return sparse_index_call(me, ix, [&](bert_ctx *ctx, SparseIndex &x, std::string &err) -> int32_t {
        if (!text_model_ok(ctx, x, err)) return -2;
        if (k < 1 || k > SparseIndex::MAX_K || kq < 1 || kq > SparseIndex::MAX_TERMS) { err = "1 <= k <= 256 and 1 <= kq <= 256 required"; return -2; }
        if (n_queries < 0 || (n_queries > 0 && (!texts || !ids || !scores))) { err = "n_queries >= 0 and texts / outputs required"; return -2; }
        if (n_queries == 0) return 0;
        // (refused before the model runs: the search itself would refuse each chunk)
        if (!x.has_postings() || x.inverted_rows() != x.size()) { err = "the postings do not cover the index's rows: call bert_hip_sparse_index_invert"; return -2; }
        std::vector<int32_t> hid((size_t)n_queries * k);
        std::vector<float> hsc((size_t)n_queries * k);
        const int32_t r = sparse_text_chunks(ctx, x, n_threads, n_queries, texts, kq, [&](int32_t i0, int32_t nb, const int32_t *d_ids, const float *d_w) -> int32_t {
            return x.search_device_to_host(nb, kq, d_ids, d_w, k, hid.data() + (size_t)i0 * k, hsc.data() + (size_t)i0 * k, err, nullptr, true);
        }, err);
        if (r != 0) { if (err.empty()) err = "device error"; return r; }
        memcpy(ids, hid.data(), hid.size() * 4);
        memcpy(scores, hsc.data(), hsc.size() * 4);
        return 0;
    });
}

int32_t bert_hip_sparse_index_rescore(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids, const float *q_weights,
                                      int32_t n_cand, const int32_t *cand_ids, int32_t k, int32_t *ids, float *scores) {
    return sparse_index_call("bert_hip_sparse_index_rescore", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) {
        return x.rescore_to_host(n_queries, kq, q_ids, q_weights, n_cand, cand_ids, k, ids, scores, err);
    });
}

int32_t bert_hip_sparse_index_rescore_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *d_q_ids,
                                             const float *d_q_weights, int32_t n_cand, const int32_t *d_cand_ids, int32_t k, int32_t *d_ids,
                                             float *d_scores, void *stream) {
    return sparse_index_call("bert_hip_sparse_index_rescore_device", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) {
        return x.rescore_device(n_queries, kq, d_q_ids, d_q_weights, n_cand, d_cand_ids, k, d_ids, d_scores, (hipStream_t)stream, err);
    });
}

int32_t bert_hip_sparse_index_remove(struct bert_hip_sparse_index *ix, int32_t n, const int32_t *ids) {
    return sparse_index_call("bert_hip_sparse_index_remove", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) { return x.remove(n, ids, err); });
}

int32_t bert_hip_sparse_index_n_live(struct bert_hip_sparse_index *ix) { return ix && ix->ix ? ix->ix->n_live() : -1; }

int32_t bert_hip_sparse_index_compact(struct bert_hip_sparse_index *ix, int32_t *old_ids) {
    return sparse_index_call("bert_hip_sparse_index_compact", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) { return x.compact(old_ids, err); });
}

int32_t bert_hip_sparse_index_save(struct bert_hip_sparse_index *ix, const char *path) {
    return sparse_index_call("bert_hip_sparse_index_save", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) -> int32_t {
        if (!path || !*path) { err = "a path is required"; return -2; }
        return x.save(path, err) ? 0 : -3;
    });
}

struct bert_hip_sparse_index *bert_hip_sparse_index_load(struct bert_ctx *ctx, const char *path) {
    return guarded("bert_hip_sparse_index_load", [&]() -> bert_hip_sparse_index * {
        const char *me = "bert_hip_sparse_index_load";
        if (!ctx) { fprintf(stderr, "%s: no context\n", me); return nullptr; }
        if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device (tokenizer-only): an index lives on the context's device\n", me); return nullptr; }
        if (!path) { fprintf(stderr, "%s: no path\n", me); return nullptr; }
        std::unique_ptr<FILE, FileCloser> f(fopen(path, "rb"));
        struct stat st;
        if (!f || fstat(fileno(f.get()), &st) != 0 || !S_ISREG(st.st_mode)) { fprintf(stderr, "%s: cannot read '%s'\n", me, path); return nullptr; }
        // everything the header promises is checked, against the file's length too, before anything is allocated
        unsigned char hdr[INDEX_HEADER_BYTES];
        const size_t got = fread(hdr, 1, sizeof hdr, f.get());
        SparseIndexFileHeader h;
        std::string err;
        if (!sparse_index_header_check(hdr, got, (uint64_t)st.st_size, h, err)) { fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str()); return nullptr; }
        std::unique_ptr<SparseIndex> ix(SparseIndex::load(ctx->engine(), f.get(), h, err));
        if (!ix) { fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str()); return nullptr; }
        std::unique_ptr<bert_hip_sparse_index> out(new bert_hip_sparse_index);
        out->ctx = ctx;
        out->ix = std::move(ix);
        ctx->sparse_indexes.push_back(out.get());
        return out.release();
    }, (bert_hip_sparse_index *)nullptr);
}

int32_t bert_hip_sparse_index_get_rows(struct bert_hip_sparse_index *ix, int32_t n, const int32_t *row_ids, int32_t *out_ids, float *out_weights) {
    return sparse_index_call("bert_hip_sparse_index_get_rows", ix, [&](bert_ctx *, SparseIndex &x, std::string &err) {
        return x.get_rows(n, row_ids, out_ids, out_weights, err);
    });
}

}  // extern "C"
