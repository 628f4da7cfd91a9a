// token_index_api.cpp — the bert_hip_token_index_* entry points of bert_hip.h: a token index (token_index.h) on a context's first
// device.  The text routes tokenize and pack as bert_hip_encode_tokens_batch does and run the token-rows pass with flags 1 | 2 (each
// row over its L2 norm, f16) in chunks of chunk_tokens: add_texts straight into the index's storage, search_texts into a device buffer
// the scan reads in place.  The rows never reach the host.  Behind them the bert_hip_late_index_* entry points: the same index's
// remove, filtered searches, compact, save and load, and the int8 form's create, dtype and get_codes (an int8 index hands add_texts a
// buffer of its own for the f16 rows and quantises from there: TokenIndex::append_room).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../../include/bert_hip.h"
#include "abi.h"
#include "token_index_file.h"

using namespace bert_hip;

namespace {

// The frame of an entry point that takes a token index: -1 (after a line on stderr) without one, else the body's result; a body
// that returns -2 or -3 has put its message into err, and it is printed here.  -4 for an exception.
template <class R = int32_t, class F>
R token_index_call(const char *me, bert_hip_token_index *ix, F &&body) {
    return guarded(me, [&]() -> R {
        if (!ix || !ix->ix) { fprintf(stderr, "%s: no index\n", me); return (R)-1; }
        std::string err;
        const R r = body(ix->ctx, *ix->ix, err);
        if ((r == -2 || r == -3) && !err.empty()) fprintf(stderr, "%s: %s\n", me, err.c_str());
        return r;
    }, (R)-4);
}

// Tokenizes the texts in groups of 4096 and cuts each group at chunk_tokens between sentences; per chunk: ids | cu_seqlens into the
// index's device buffer, then use(i0, nb, T, max_len, h_cu, d_ids, d_cu) — h_cu: the chunk's lengths from 0, host; d_ids / d_cu: the
// same on the device — all on the index's stream, which is synchronised behind every chunk.  limit > 0: a text of more tokens is
// refused (-2).  0, -2 or -3 (+ err).
template <class F>
int32_t token_text_chunks(bert_ctx *ctx, TokenIndex &x, int32_t n_threads, int32_t n, const char **texts, int limit, size_t out_row_bytes, F &&use,
                          std::string &err) {
    constexpr int32_t GROUP = 4096;
    Engine *eng = ctx->engine();
    TokenGroup &g = ctx->texts.group[0];
    std::vector<int32_t> h_cu;
    for (int32_t i0 = 0; i0 < n; i0 += GROUP) {
        const int32_t m = std::min(GROUP, n - i0);
        g.tokenize(ctx->texts, n_threads, m, texts + i0);
        if (g.n_ok < m) { err = "input " + std::to_string(i0 + g.n_ok) + " cannot be evaluated"; return -2; }
        const int32_t *cu = g.cu.data();
        if (limit > 0)
            for (int b = 0; b < m; ++b)
                if (cu[b + 1] - cu[b] > limit) {
                    err = "query " + std::to_string(i0 + b) + " has " + std::to_string(cu[b + 1] - cu[b]) + " tokens; a search at this dim takes at most " + std::to_string(limit);
                    return -2;
                }
        for (int b0 = 0; b0 < m;) {
            int b1 = b0 + 1, max_len = cu[b0 + 1] - cu[b0];
            while (b1 < m && cu[b1 + 1] - cu[b0] <= eng->options().chunk_tokens) { max_len = std::max(max_len, cu[b1 + 1] - cu[b1]); ++b1; }
            const int nb = b1 - b0, T = cu[b1] - cu[b0];
            const size_t off_cu = ((size_t)T * 4 + 15) & ~(size_t)15;
            char *d_in = nullptr, *d_out = nullptr;
            if (!x.text_buffers(off_cu + (size_t)(nb + 1) * 4, (size_t)T * out_row_bytes, d_in, d_out, err)) return -3;
            h_cu.resize(nb + 1);
            for (int j = 0; j <= nb; ++j) h_cu[j] = cu[b0 + j] - cu[b0];
            hipStream_t s = x.stream();
            // (pageable sources: both copies have left the host buffers when they return)
            if (hipMemcpyAsync(d_in, g.packed.get() + cu[b0], (size_t)T * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync(d_in + off_cu, h_cu.data(), (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
                (void)hipStreamSynchronize(s);
                err = "hipMemcpyAsync (ids) failed";
                return -3;
            }
            int32_t r = use(i0 + b0, nb, T, max_len, h_cu.data(), (const int32_t *)d_in, (const int32_t *)(d_in + off_cu), d_out);
            if (hipStreamSynchronize(s) != hipSuccess && r == 0) { err = "device error"; r = -3; }
            if (r != 0) return r;
            b0 = b1;
        }
    }
    return 0;
}

// an allow-list of n_words words covers the index (-2 + err otherwise)
bool allow_ok(const TokenIndex &x, const uint32_t *allow, int32_t n_words, std::string &err) {
    const int64_t need = ((int64_t)x.size() + 31) / 32;
    if (!allow || n_words >= need) return true;
    err = "the allow-list has " + std::to_string(n_words) + " words, an index of " + std::to_string(x.size()) + " documents needs " + std::to_string(need);
    return false;
}

// what the text routes ask of the index (false + err otherwise)
bool text_dim_ok(const bert_ctx *ctx, const TokenIndex &x, std::string &err) {
    if (x.dim() == ctx->hp.n_embd) return true;
    err = "the index has dim " + std::to_string(x.dim()) + ", the model's n_embd is " + std::to_string(ctx->hp.n_embd);
    return false;
}

// bert_hip_token_index_create (dtype 1) and bert_hip_late_index_create
bert_hip_token_index *create_token_index(const char *me, bert_ctx *ctx, int32_t dim, int32_t dtype) {
    return guarded(me, [&]() -> bert_hip_token_index * {
        if (!ctx) { fprintf(stderr, "%s: no context\n", me); return nullptr; }
        if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device (tokenizer-only): an index lives on the context's device\n", me); return nullptr; }
        if (dim == 0) dim = ctx->hp.n_embd;
        std::string err;
        std::unique_ptr<TokenIndex> ix(TokenIndex::create(ctx->engine(), dim, dtype, err));
        if (!ix) { fprintf(stderr, "%s: %s\n", me, err.c_str()); return nullptr; }
        std::unique_ptr<bert_hip_token_index> h(new bert_hip_token_index);
        h->ctx = ctx;
        h->ix = std::move(ix);
        ctx->token_indexes.push_back(h.get());
        return h.release();
    }, (bert_hip_token_index *)nullptr);
}

}  // namespace

extern "C" {

struct bert_hip_token_index *bert_hip_token_index_create(struct bert_ctx *ctx, int32_t dim) {
    return create_token_index("bert_hip_token_index_create", ctx, dim, 1);
}

void bert_hip_token_index_free(struct bert_hip_token_index *ix) {
    guarded("bert_hip_token_index_free", [&] {
        if (!ix) return;
        auto &v = ix->ctx->token_indexes;
        v.erase(std::remove(v.begin(), v.end(), ix), v.end());
        delete ix;
    });
}

int32_t bert_hip_token_index_size(struct bert_hip_token_index *ix) { return ix && ix->ix ? ix->ix->size() : -1; }

int64_t bert_hip_token_index_n_tokens(struct bert_hip_token_index *ix) { return ix && ix->ix ? ix->ix->n_tokens() : -1; }

int32_t bert_hip_token_index_max_query_tokens(struct bert_hip_token_index *ix) { return ix && ix->ix ? ix->ix->max_query_tokens() : -1; }

int32_t bert_hip_token_index_reserve(struct bert_hip_token_index *ix, int32_t n_docs, int64_t n_tokens, int32_t n_queries, int32_t max_q_len, int32_t k) {
    return token_index_call("bert_hip_token_index_reserve", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.reserve(n_docs, n_tokens, n_queries, max_q_len, k, err);
    });
}

int32_t bert_hip_token_index_add(struct bert_hip_token_index *ix, int32_t n_docs, const int32_t *cu, const float *rows) {
    return token_index_call("bert_hip_token_index_add", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t { return x.add_host(n_docs, cu, rows, err); });
}

int32_t bert_hip_token_index_add_device(struct bert_hip_token_index *ix, int32_t n_docs, const int32_t *cu, const void *d_rows, void *stream) {
    return token_index_call("bert_hip_token_index_add_device", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.add_device(n_docs, cu, (const half_t *)d_rows, (hipStream_t)stream, err);
    });
}

int32_t bert_hip_token_index_add_texts(struct bert_hip_token_index *ix, int32_t n_threads, int32_t n, const char **texts) {
    return token_index_call("bert_hip_token_index_add_texts", ix, [&](bert_ctx *ctx, TokenIndex &x, std::string &err) -> int32_t {
        if (!text_dim_ok(ctx, x, err)) return -2;
        if (n < 0 || (n > 0 && !texts)) { err = "n >= 0 and texts required"; return -2; }
        const int first = x.size();
        if (n == 0) return first;
        Engine *eng = ctx->engine();
        const int32_t r = token_text_chunks(ctx, x, n_threads, n, texts, 0, 0,
            [&](int32_t, int32_t nb, int32_t T, int32_t max_len, const int32_t *h_cu, const int32_t *d_ids, const int32_t *d_cu, char *) -> int32_t {
                half_t *dst = x.append_room(T, err);
                if (!dst) return err.rfind("add:", 0) == 0 ? -2 : -3;
                if (eng->eval_packed_device(d_ids, d_cu, nb, T, max_len, nullptr, x.stream(), nullptr, err, nullptr, 0, 0, -1, dst,
                                            TOKEN_ROWS_NORMALIZE | TOKEN_ROWS_F16) != 0) return -3;
                const int32_t a = x.add_in_place(nb, h_cu, err);
                return a < 0 ? a : 0;
            }, err);
        if (r == 0) return first;
        x.truncate(first);
        if (err.empty()) err = "device error";
        return r;
    });
}

int32_t bert_hip_token_index_get_doc(struct bert_hip_token_index *ix, int32_t id, float *rows, int32_t cap_tokens) {
    return token_index_call("bert_hip_token_index_get_doc", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t { return x.get_doc(id, rows, cap_tokens, err); });
}

int32_t bert_hip_token_index_search(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *qcu, const float *q_rows, int32_t k, int32_t *ids,
                                    float *scores) {
    return token_index_call("bert_hip_token_index_search", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.search_host(n_queries, qcu, q_rows, k, ids, scores, err);
    });
}

int32_t bert_hip_token_index_search_device(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *d_qcu, const void *d_q, int32_t max_q_len,
                                           int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    return token_index_call("bert_hip_token_index_search_device", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.search_device(n_queries, d_qcu, (const half_t *)d_q, max_q_len, k, d_ids, d_scores, (hipStream_t)stream, err);
    });
}

int32_t bert_hip_token_index_search_texts(struct bert_hip_token_index *ix, int32_t n_threads, int32_t n_queries, const char **texts, int32_t k, int32_t *ids,
                                          float *scores) {
    return token_index_call("bert_hip_token_index_search_texts", ix, [&](bert_ctx *ctx, TokenIndex &x, std::string &err) -> int32_t {
        if (!text_dim_ok(ctx, x, err)) return -2;
        if (k < 1 || k > TokenIndex::MAX_K) { err = "1 <= k <= 256 required"; return -2; }
        if (n_queries < 0 || (n_queries > 0 && (!texts || !ids || !scores))) { err = "n_queries >= 0 and texts / outputs required"; return -2; }
        if (n_queries == 0) return 0;
        Engine *eng = ctx->engine();
        // (the outputs are written only when every chunk has succeeded)
        std::vector<int32_t> hid((size_t)n_queries * k);
        std::vector<float> hsc((size_t)n_queries * k);
        const int32_t r = token_text_chunks(ctx, x, n_threads, n_queries, texts, x.max_query_tokens(), (size_t)x.dim() * 2,
            [&](int32_t i0, int32_t nb, int32_t T, int32_t max_len, const int32_t *, const int32_t *d_ids, const int32_t *d_cu, char *d_out) -> int32_t {
                if (eng->eval_packed_device(d_ids, d_cu, nb, T, max_len, nullptr, x.stream(), nullptr, err, nullptr, 0, 0, -1, d_out,
                                            TOKEN_ROWS_NORMALIZE | TOKEN_ROWS_F16) != 0) return -3;
                return x.search_device_to_host(nb, d_cu, (const half_t *)d_out, max_len, k, hid.data() + (size_t)i0 * k, hsc.data() + (size_t)i0 * k, err);
            }, err);
        if (r != 0) { if (err.empty()) err = "device error"; return r; }
        memcpy(ids, hid.data(), hid.size() * 4);
        memcpy(scores, hsc.data(), hsc.size() * 4);
        return 0;
    });
}

int32_t bert_hip_token_index_rescore(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *qcu, const float *q_rows, int32_t n_cand,
                                     const int32_t *cand_ids, int32_t k, int32_t *ids, float *scores) {
    return token_index_call("bert_hip_token_index_rescore", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.rescore_host(n_queries, qcu, q_rows, n_cand, cand_ids, k, ids, scores, err);
    });
}

int32_t bert_hip_token_index_rescore_device(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *d_qcu, const void *d_q, int32_t n_cand,
                                            const int32_t *d_cand_ids, int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    return token_index_call("bert_hip_token_index_rescore_device", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.rescore_device(n_queries, d_qcu, (const half_t *)d_q, n_cand, d_cand_ids, k, d_ids, d_scores, (hipStream_t)stream, err);
    });
}

// ------------------------------------------------------------------------------------------------
// bert_hip_late_index_*: the token index's life cycle (bert_hip.h "LATE INDEX").  Frames around the class; load checks the file's header
// (token_index_file.h) before it makes the index.
// ------------------------------------------------------------------------------------------------
int32_t bert_hip_late_index_remove(struct bert_hip_token_index *ix, int32_t n, const int32_t *ids) {
    return token_index_call("bert_hip_late_index_remove", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t { return x.remove(n, ids, err); });
}

int32_t bert_hip_late_index_n_live(struct bert_hip_token_index *ix) { return ix && ix->ix ? ix->ix->n_live() : -1; }

int64_t bert_hip_late_index_n_live_tokens(struct bert_hip_token_index *ix) { return ix && ix->ix ? ix->ix->n_live_tokens() : -1; }

int32_t bert_hip_late_index_search_filtered(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *qcu, const float *q_rows, int32_t k,
                                            const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores) {
    return token_index_call("bert_hip_late_index_search_filtered", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        if (!allow_ok(x, allow, n_words, err)) return -2;
        return x.search_host(n_queries, qcu, q_rows, k, ids, scores, err, allow);
    });
}

int32_t bert_hip_late_index_search_filtered_device(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *d_qcu, const void *d_q,
                                                   int32_t max_q_len, int32_t k, const uint32_t *d_allow, int32_t n_words, int32_t *d_ids,
                                                   float *d_scores, void *stream) {
    return token_index_call("bert_hip_late_index_search_filtered_device", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        if (!allow_ok(x, d_allow, n_words, err)) return -2;
        return x.search_device(n_queries, d_qcu, (const half_t *)d_q, max_q_len, k, d_ids, d_scores, (hipStream_t)stream, err, d_allow);
    });
}

int32_t bert_hip_late_index_compact(struct bert_hip_token_index *ix, int32_t *old_ids) {
    return token_index_call("bert_hip_late_index_compact", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t { return x.compact(old_ids, err); });
}

int32_t bert_hip_late_index_save(struct bert_hip_token_index *ix, const char *path) {
    return token_index_call("bert_hip_late_index_save", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        if (!path || !*path) { err = "a path is required"; return -2; }
        if (x.dtype() == 2) { err = "save: not available for an int8 token index"; return -2; }
        return x.save(path, err) ? 0 : -3;
    });
}

struct bert_hip_token_index *bert_hip_late_index_load(struct bert_ctx *ctx, const char *path) {
    return guarded("bert_hip_late_index_load", [&]() -> bert_hip_token_index * {
        const char *me = "bert_hip_late_index_load";
        if (!ctx) { fprintf(stderr, "%s: no context\n", me); return nullptr; }
        if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device (tokenizer-only): an index lives on the context's device\n", me); return nullptr; }
        if (!path) { fprintf(stderr, "%s: no path\n", me); return nullptr; }
        std::unique_ptr<FILE, FileCloser> f(fopen(path, "rb"));
        struct stat st;
        if (!f || fstat(fileno(f.get()), &st) != 0 || !S_ISREG(st.st_mode)) { fprintf(stderr, "%s: cannot read '%s'\n", me, path); return nullptr; }
        // everything the header promises is checked, against the file's length too, before anything is allocated
        unsigned char hdr[INDEX_HEADER_BYTES];
        const size_t got = fread(hdr, 1, sizeof hdr, f.get());
        TokenIndexFileHeader h;
        std::string err;
        if (!token_index_header_check(hdr, got, (uint64_t)st.st_size, h, err)) { fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str()); return nullptr; }
        std::unique_ptr<TokenIndex> ix(TokenIndex::load(ctx->engine(), f.get(), h, err));
        if (!ix) { fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str()); return nullptr; }
        std::unique_ptr<bert_hip_token_index> out(new bert_hip_token_index);
        out->ctx = ctx;
        out->ix = std::move(ix);
        ctx->token_indexes.push_back(out.get());
        return out.release();
    }, (bert_hip_token_index *)nullptr);
}

// ------------------------------------------------------------------------------------------------
// the int8 form (bert_hip.h "TOKEN INDEX, int8 form"): every entry point above takes such an index as it takes an f16 one
// ------------------------------------------------------------------------------------------------
struct bert_hip_token_index *bert_hip_late_index_create(struct bert_ctx *ctx, int32_t dim, int32_t dtype) {
    return create_token_index("bert_hip_late_index_create", ctx, dim, dtype);
}

int32_t bert_hip_late_index_dtype(struct bert_hip_token_index *ix) { return ix && ix->ix ? ix->ix->dtype() : -1; }

int32_t bert_hip_late_index_get_codes(struct bert_hip_token_index *ix, int32_t id, int8_t *codes, float *scales, int32_t cap_tokens) {
    return token_index_call("bert_hip_late_index_get_codes", ix, [&](bert_ctx *, TokenIndex &x, std::string &err) -> int32_t {
        return x.get_codes(id, codes, scales, cap_tokens, err);
    });
}

}  // extern "C"
