// index_api.cpp — the bert_hip_index_* entry points of bert_hip.h: an embedding index (search.h) on a context's first device.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../../include/bert_hip.h"
#include "abi.h"
#include "index_file.h"
#include "text_routes.h"

using namespace bert_hip;

namespace {

// The frame of an entry point that takes an index: -1 (after a line on stderr) without one, else the body's result; a body
// that returns -3 has put its message into err, and it is printed here.  -4 for an exception.
template <class F>
int32_t index_call(const char *me, bert_hip_index *ix, F &&body) {
    return guarded(me, [&]() -> int32_t {
        if (!ix || !ix->ix) { fprintf(stderr, "%s: no index\n", me); return -1; }
        std::string err;
        const int32_t r = body(ix->ctx, *ix->ix, err);
        if (r == -3) fprintf(stderr, "%s: %s\n", me, err.c_str());
        return r;
    }, (int32_t)-4);
}

// (the text routes' way from texts to the index's scratch buffer, encode_groups_device and encode_host: text_routes.h)

// (-2 after a line on stderr: the index does not hold this model's embeddings)
bool dim_ok(const char *me, const bert_ctx *ctx, const Index &x) {
    if (x.dim() != ctx->hp.n_embd) fprintf(stderr, "%s: the index has dim %d, the model's embeddings %d\n", me, x.dim(), ctx->hp.n_embd);
    return x.dim() == ctx->hp.n_embd;
}

// an allow-list of n_words words covers the index (-2 after a line on stderr otherwise)
bool allow_ok(const char *me, const Index &x, const uint32_t *allow, int32_t n_words) {
    const int64_t need = ((int64_t)x.size() + 31) / 32;
    if (allow && n_words < need) fprintf(stderr, "%s: the allow-list has %d words, an index of %d rows needs %lld\n", me, n_words, x.size(), (long long)need);
    return !allow || n_words >= need;
}

// the shape of a rescore call (-2 after a line on stderr otherwise); have_ptrs: every pointer the call needs is there
bool rescore_args_ok(const char *me, int32_t n_queries, int32_t n_cand, int32_t k, bool have_ptrs) {
    const bool ok = k >= 1 && k <= Index::MAX_K && n_cand >= 1 && n_cand <= Index::MAX_CAND && n_queries >= 0 && (n_queries == 0 || have_ptrs);
    if (!ok) fprintf(stderr, "%s: 1 <= k <= 256, 1 <= n_cand <= 1024, n_queries >= 0 and queries / candidates / outputs required\n", me);
    return ok;
}

// what a two-stage search asks of its two indexes and its shape (-2 after a line on stderr otherwise)
bool two_stage_ok(const char *me, const bert_hip_index *coarse, const bert_hip_index *fine, int32_t n_queries, int32_t n_cand, int32_t k,
                  bool have_ptrs) {
    const char *why = nullptr;
    if (!coarse || !coarse->ix) why = "no coarse index";
    else if (coarse->ctx != fine->ctx) why = "the two indexes belong to different contexts";
    else if (coarse->ix->dim() != fine->ix->dim()) why = "the two indexes differ in dim";
    else if (coarse->ix->size() != fine->ix->size()) why = "the two indexes differ in size";
    else if (k < 1 || k > n_cand || n_cand > Index::MAX_K) why = "1 <= k <= n_cand <= 256 required";
    else if (n_queries < 0 || (n_queries > 0 && !have_ptrs)) why = "n_queries >= 0 and queries / outputs required";
    if (why) fprintf(stderr, "%s: %s\n", me, why);
    return !why;
}

// what a probed two-stage search asks on top of two_stage_ok: coarse's partition and nprobe, and an allow-list that covers coarse
bool two_stage_probed_ok(const char *me, const Index &coarse, int32_t nprobe, const uint32_t *allow, int32_t n_words) {
    const char *why = nullptr;
    if (coarse.n_lists() == 0) why = "the coarse index has no partition";
    else if (nprobe < 1 || nprobe > std::min(coarse.n_lists(), Index::MAX_K)) why = "1 <= nprobe <= min(n_lists, 256) required";
    if (why) fprintf(stderr, "%s: %s\n", me, why);
    return !why && allow_ok(me, coarse, allow, n_words);
}

// the shape of a probed search (-2 after a line on stderr otherwise)
bool probed_ok(const char *me, const Index &x, int32_t n_queries, int32_t nprobe, int32_t k, bool have_ptrs) {
    const char *why = nullptr;
    if (x.n_lists() == 0) why = "the index has no partition";
    else if (nprobe < 1 || nprobe > std::min(x.n_lists(), Index::MAX_K)) why = "1 <= nprobe <= min(n_lists, 256) required";
    else if (k < 1 || k > Index::MAX_K) why = "k must be 1 .. 256";
    else if (n_queries < 0 || (n_queries > 0 && !have_ptrs)) why = "n_queries >= 0 and queries / outputs required";
    if (why) fprintf(stderr, "%s: %s\n", me, why);
    return !why;
}

// centroids [n_lists][dim] as partition and kmeans take them (-2 after a line on stderr otherwise)
bool centroids_ok(const char *me, const Index &x, int32_t n_lists, const float *centroids) {
    const char *why = nullptr;
    if (n_lists < 1 || n_lists > Index::MAX_LISTS) why = "1 <= n_lists <= 65536 required";
    else if (!centroids) why = "centroids required";
    else
        for (size_t i = 0; i < (size_t)n_lists * x.dim() && !why; ++i)
            if (!std::isfinite(centroids[i])) why = "a centroid element is not finite";
    if (why) fprintf(stderr, "%s: %s\n", me, why);
    return !why;
}

}  // namespace

extern "C" {

struct bert_hip_index *bert_hip_index_create(struct bert_ctx *ctx, int32_t dim, int32_t dtype) {
    return guarded("bert_hip_index_create", [&]() -> bert_hip_index * {
        const char *me = "bert_hip_index_create";
        if (!ctx) { fprintf(stderr, "%s: no context\n", me); return nullptr; }
        if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device (tokenizer-only): an index lives on the context's device\n", me); return nullptr; }
        if (dim == 0) dim = ctx->hp.n_embd;
        std::string err;
        std::unique_ptr<Index> ix(Index::create(ctx->engine(), dim, dtype, err));
        if (!ix) { fprintf(stderr, "%s: %s\n", me, err.c_str()); return nullptr; }
        std::unique_ptr<bert_hip_index> h(new bert_hip_index);
        h->ctx = ctx;
        h->ix = std::move(ix);
        ctx->indexes.push_back(h.get());
        return h.release();
    }, (bert_hip_index *)nullptr);
}

void bert_hip_index_free(struct bert_hip_index *ix) {
    guarded("bert_hip_index_free", [&] {
        if (!ix) return;
        auto &v = ix->ctx->indexes;
        v.erase(std::remove(v.begin(), v.end(), ix), v.end());
        delete ix;
    });
}

int32_t bert_hip_index_size(struct bert_hip_index *ix) { return ix && ix->ix ? ix->ix->size() : -1; }

int32_t bert_hip_index_reserve(struct bert_hip_index *ix, int32_t n_rows, int32_t n_queries, int32_t k) {
    return index_call("bert_hip_index_reserve", ix, [&](bert_ctx *, Index &x, std::string &err) { return x.reserve(n_rows, n_queries, k, err) ? 0 : -3; });
}

int32_t bert_hip_index_add(struct bert_hip_index *ix, int32_t n, const float *rows) {
    return index_call("bert_hip_index_add", ix, [&](bert_ctx *, Index &x, std::string &err) {
        const int first = x.add_host(n, rows, err);
        return first < 0 ? -3 : first;
    });
}

int32_t bert_hip_index_add_device(struct bert_hip_index *ix, int32_t n, const float *d_rows, void *stream) {
    return index_call("bert_hip_index_add_device", ix, [&](bert_ctx *, Index &x, std::string &err) {
        const int first = x.add_device(n, d_rows, (hipStream_t)stream, err);
        return first < 0 ? -3 : first;
    });
}

int32_t bert_hip_index_add_texts(struct bert_hip_index *ix, int32_t n_threads, int32_t n, const char **texts) {
    const char *me = "bert_hip_index_add_texts";
    return index_call(me, ix, [&](bert_ctx *ctx, Index &x, std::string &err) -> int32_t {
        if (!dim_ok(me, ctx, x)) return -2;
        if (n < 0 || (n > 0 && !texts)) { fprintf(stderr, "%s: n >= 0 and texts required\n", me); return -2; }
        const int first = x.size();
        if (n == 0) return first;
        bool ok;
        if (ctx->engines.size() > 1) {
            std::vector<float> emb;
            ok = encode_host(ctx, n_threads, n, texts, emb, err) && x.add_host(n, emb.data(), err) >= 0;
        } else {
            ok = encode_groups_device(ctx, x, n_threads, n, texts, [&](int32_t, int32_t c, const float *d) {
                return x.add_device(c, d, x.stream(), err) >= 0 && hipStreamSynchronize(x.stream()) == hipSuccess;
            }, err);
        }
        if (ok) return first;
        x.truncate(first);
        if (err.empty()) err = "device error";
        return -3;
    });
}

int32_t bert_hip_index_add_long_texts(struct bert_hip_index *ix, int32_t n_threads, int32_t n, const char **texts, int32_t window, int32_t stride) {
    const char *me = "bert_hip_index_add_long_texts";
    return index_call(me, ix, [&](bert_ctx *ctx, Index &x, std::string &err) -> int32_t {
        if (!dim_ok(me, ctx, x) || !long_args_ok(me, ctx, window, stride)) return -2;
        if (n < 0 || (n > 0 && !texts)) { fprintf(stderr, "%s: n >= 0 and texts required\n", me); return -2; }
        const int first = x.size();
        if (n == 0) return first;
        const size_t H = ctx->hp.n_embd;
        bool ok;
        if (ctx->engines.size() > 1) {
            // (through the host, as add_texts does)
            std::vector<float> emb((size_t)n * H);
            std::vector<float *> rows((size_t)n);
            for (int32_t i = 0; i < n; ++i) rows[i] = emb.data() + i * H;
            ok = encode_long_batch_impl(ctx, n_threads, n, texts, window, stride, rows.data(), nullptr) == n && x.add_host(n, emb.data(), err) >= 0;
            if (!ok && err.empty()) err = "the texts could not be encoded";
        } else {
            // every group's pooled rows go from the device buffer straight into the index
            ok = ctx->texts.encode_long_groups(n_threads, n, texts, window, stride, nullptr, [&](const LongGroup &g, int32_t) -> int32_t {
                const int32_t G = g.n_texts();
                float *d = x.scratch((size_t)G * H, err);
                if (!d || ctx->engine()->eval_packed_grouped_host(g.packed.data(), g.cu.data(), g.n_windows(), g.group_cu.data(), G, nullptr, d, err) != 0) return -1;
                return x.add_device(G, d, x.stream(), err) >= 0 && hipStreamSynchronize(x.stream()) == hipSuccess ? G : -1;
            }) == n;
        }
        if (ok) return first;
        x.truncate(first);
        if (err.empty()) err = "device error";
        return -3;
    });
}

int32_t bert_hip_index_search(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t k, int32_t *ids, float *scores) {
    return index_call("bert_hip_index_search", ix, [&](bert_ctx *, Index &x, std::string &err) {
        return x.search_to_host(n_queries, queries, false, k, ids, scores, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t k, int32_t *d_ids,
                                     float *d_scores, void *stream) {
    return index_call("bert_hip_index_search_device", ix, [&](bert_ctx *, Index &x, std::string &err) {
        return x.search_device(n_queries, d_queries, k, d_ids, d_scores, (hipStream_t)stream, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_filtered(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t k, const uint32_t *allow,
                                       int32_t n_words, int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_search_filtered";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!allow_ok(me, x, allow, n_words)) return -2;
        return x.search_to_host(n_queries, queries, false, k, ids, scores, err, allow) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_filtered_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t k,
                                              const uint32_t *d_allow, int32_t n_words, int32_t *d_ids, float *d_scores, void *stream) {
    const char *me = "bert_hip_index_search_filtered_device";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!allow_ok(me, x, d_allow, n_words)) return -2;
        return x.search_device(n_queries, d_queries, k, d_ids, d_scores, (hipStream_t)stream, err, d_allow) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_rescore(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t n_cand, const int32_t *cand_ids,
                               int32_t k, int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_rescore";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!rescore_args_ok(me, n_queries, n_cand, k, queries && cand_ids && ids && scores)) return -2;
        for (size_t i = 0; i < (size_t)n_queries * n_cand; ++i)
            if (cand_ids[i] < -1 || cand_ids[i] >= x.size()) {
                fprintf(stderr, "%s: candidate id %d is outside [-1, %d)\n", me, cand_ids[i], x.size());
                return -2;
            }
        return x.rescore_to_host(n_queries, queries, n_cand, cand_ids, k, ids, scores, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_rescore_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t n_cand,
                                      const int32_t *d_cand_ids, int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    const char *me = "bert_hip_index_rescore_device";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!rescore_args_ok(me, n_queries, n_cand, k, d_queries && d_cand_ids && d_ids && d_scores)) return -2;
        return x.rescore_device(n_queries, d_queries, n_cand, d_cand_ids, k, d_ids, d_scores, (hipStream_t)stream, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_rescored(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries, const float *queries,
                                       int32_t n_cand, int32_t k, int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_search_rescored";
    return index_call(me, fine, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!two_stage_ok(me, coarse, fine, n_queries, n_cand, k, queries && ids && scores)) return -2;
        return x.search_rescored_to_host(*coarse->ix, n_queries, queries, n_cand, k, ids, scores, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_rescored_device(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries,
                                              const float *d_queries, int32_t n_cand, int32_t k, int32_t *d_ids, float *d_scores, void *stream) {
    const char *me = "bert_hip_index_search_rescored_device";
    return index_call(me, fine, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!two_stage_ok(me, coarse, fine, n_queries, n_cand, k, d_queries && d_ids && d_scores)) return -2;
        return x.search_rescored_device(*coarse->ix, n_queries, d_queries, n_cand, k, d_ids, d_scores, (hipStream_t)stream, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_get_rows(struct bert_hip_index *ix, int32_t n, const int32_t *ids, float *rows) {
    const char *me = "bert_hip_index_get_rows";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (n < 0 || (n > 0 && (!ids || !rows))) { fprintf(stderr, "%s: n >= 0 and ids / rows required\n", me); return -2; }
        for (int32_t i = 0; i < n; ++i)
            if (ids[i] < 0 || ids[i] >= x.size()) { fprintf(stderr, "%s: id %d is outside [0, %d)\n", me, ids[i], x.size()); return -2; }
        // (into a buffer of our own: the caller's rows stay untouched on an error)
        std::vector<float> out((size_t)n * x.dim());
        if (x.get_rows(n, ids, out.data(), err) != 0) return -3;
        memcpy(rows, out.data(), out.size() * 4);
        return 0;
    });
}

int32_t bert_hip_index_partition(struct bert_hip_index *ix, int32_t n_lists, const float *centroids) {
    const char *me = "bert_hip_index_partition";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (n_lists != 0 && !centroids_ok(me, x, n_lists, centroids)) return -2;
        return x.partition(n_lists, centroids, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_n_lists(struct bert_hip_index *ix) { return ix && ix->ix ? ix->ix->n_lists() : -1; }

int32_t bert_hip_index_partition_centroids(struct bert_hip_index *ix, float *centroids) {
    const char *me = "bert_hip_index_partition_centroids";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &) -> int32_t {
        if (x.n_lists() == 0 || !centroids) { fprintf(stderr, "%s: a partition and room for its centroids required\n", me); return -2; }
        memcpy(centroids, x.centroids().data(), x.centroids().size() * 4);
        return 0;
    });
}

int32_t bert_hip_index_partition_lists(struct bert_hip_index *ix, int32_t *list_of_row) {
    const char *me = "bert_hip_index_partition_lists";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &) -> int32_t {
        if (x.n_lists() == 0 || (x.size() > 0 && !list_of_row)) { fprintf(stderr, "%s: a partition and room for size entries required\n", me); return -2; }
        x.partition_lists(list_of_row);
        return 0;
    });
}

int32_t bert_hip_index_kmeans(struct bert_hip_index *ix, int32_t n_lists, int32_t n_iter, float *centroids) {
    const char *me = "bert_hip_index_kmeans";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!centroids_ok(me, x, n_lists, centroids)) return -2;
        if (n_iter < 1) { fprintf(stderr, "%s: n_iter >= 1 required\n", me); return -2; }
        // (refined in a buffer of our own: the caller's centroids stay untouched on an error)
        std::vector<float> c(centroids, centroids + (size_t)n_lists * x.dim());
        if (x.kmeans(n_lists, n_iter, c.data(), err) != 0) return -3;
        memcpy(centroids, c.data(), c.size() * 4);
        return 0;
    });
}

int32_t bert_hip_index_search_probed(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t nprobe, int32_t k,
                                     int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_search_probed";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!probed_ok(me, x, n_queries, nprobe, k, queries && ids && scores)) return -2;
        return x.search_probed_to_host(n_queries, queries, nprobe, k, ids, scores, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_probed_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t nprobe, int32_t k,
                                            int32_t *d_ids, float *d_scores, void *stream) {
    const char *me = "bert_hip_index_search_probed_device";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!probed_ok(me, x, n_queries, nprobe, k, d_queries && d_ids && d_scores)) return -2;
        return x.search_probed_device(n_queries, d_queries, nprobe, k, d_ids, d_scores, (hipStream_t)stream, err) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_probed_filtered(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t nprobe, int32_t k,
                                              const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_search_probed_filtered";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!probed_ok(me, x, n_queries, nprobe, k, queries && ids && scores) || !allow_ok(me, x, allow, n_words)) return -2;
        return x.search_probed_to_host(n_queries, queries, nprobe, k, ids, scores, err, allow) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_probed_filtered_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t nprobe,
                                                     int32_t k, const uint32_t *d_allow, int32_t n_words, int32_t *d_ids, float *d_scores,
                                                     void *stream) {
    const char *me = "bert_hip_index_search_probed_filtered_device";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!probed_ok(me, x, n_queries, nprobe, k, d_queries && d_ids && d_scores) || !allow_ok(me, x, d_allow, n_words)) return -2;
        return x.search_probed_device(n_queries, d_queries, nprobe, k, d_ids, d_scores, (hipStream_t)stream, err, d_allow) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_rescored_probed(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries,
                                              const float *queries, int32_t nprobe, int32_t n_cand, int32_t k, const uint32_t *allow,
                                              int32_t n_words, int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_search_rescored_probed";
    return index_call(me, fine, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!two_stage_ok(me, coarse, fine, n_queries, n_cand, k, queries && ids && scores) ||
            !two_stage_probed_ok(me, *coarse->ix, nprobe, allow, n_words)) return -2;
        return x.search_rescored_to_host(*coarse->ix, n_queries, queries, n_cand, k, ids, scores, err, nprobe, allow) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_search_rescored_probed_device(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries,
                                                     const float *d_queries, int32_t nprobe, int32_t n_cand, int32_t k,
                                                     const uint32_t *d_allow, int32_t n_words, int32_t *d_ids, float *d_scores, void *stream) {
    const char *me = "bert_hip_index_search_rescored_probed_device";
    return index_call(me, fine, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!two_stage_ok(me, coarse, fine, n_queries, n_cand, k, d_queries && d_ids && d_scores) ||
            !two_stage_probed_ok(me, *coarse->ix, nprobe, d_allow, n_words)) return -2;
        return x.search_rescored_device(*coarse->ix, n_queries, d_queries, n_cand, k, d_ids, d_scores, (hipStream_t)stream, err, nprobe, d_allow) != 0 ? -3 : 0;
    });
}

int32_t bert_hip_index_partition_save(struct bert_hip_index *ix, const char *path) {
    const char *me = "bert_hip_index_partition_save";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (x.n_lists() == 0 || !path || !*path) { fprintf(stderr, "%s: a partition and a path required\n", me); return -2; }
        return x.save_partition(path, err) ? 0 : -3;
    });
}

int32_t bert_hip_index_partition_load(struct bert_hip_index *ix, const char *path) {
    const char *me = "bert_hip_index_partition_load";
    return index_call(me, ix, [&](bert_ctx *, Index &x, std::string &err) -> int32_t {
        if (!path || !*path) { fprintf(stderr, "%s: a path required\n", me); return -2; }
        const int r = x.load_partition(path, err);
        if (r == -2) fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str());
        return r;
    });
}

int32_t bert_hip_index_remove(struct bert_hip_index *ix, int32_t n, const int32_t *ids) {
    return index_call("bert_hip_index_remove", ix, [&](bert_ctx *, Index &x, std::string &err) {
        const int r = x.remove(n, ids, err);
        return r < 0 ? -3 : r;
    });
}

int32_t bert_hip_index_n_live(struct bert_hip_index *ix) { return ix && ix->ix ? ix->ix->n_live() : -1; }

int32_t bert_hip_index_compact(struct bert_hip_index *ix, int32_t *old_ids) {
    return index_call("bert_hip_index_compact", ix, [&](bert_ctx *, Index &x, std::string &err) {
        const int r = x.compact(old_ids, err);
        return r < 0 ? -3 : r;
    });
}

int32_t bert_hip_index_save(struct bert_hip_index *ix, const char *path) {
    return index_call("bert_hip_index_save", ix, [&](bert_ctx *, Index &x, std::string &err) { return x.save(path, err) ? 0 : -3; });
}

struct bert_hip_index *bert_hip_index_load(struct bert_ctx *ctx, const char *path) {
    return guarded("bert_hip_index_load", [&]() -> bert_hip_index * {
        const char *me = "bert_hip_index_load";
        if (!ctx) { fprintf(stderr, "%s: no context\n", me); return nullptr; }
        if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device (tokenizer-only): an index lives on the context's device\n", me); return nullptr; }
        if (!path) { fprintf(stderr, "%s: no path\n", me); return nullptr; }
        std::unique_ptr<FILE, FileCloser> f(fopen(path, "rb"));
        struct stat st;
        if (!f || fstat(fileno(f.get()), &st) != 0 || !S_ISREG(st.st_mode)) { fprintf(stderr, "%s: cannot read '%s'\n", me, path); return nullptr; }
        // everything the header promises is checked, against the file's length too, before anything is allocated
        unsigned char hdr[INDEX_HEADER_BYTES];
        const size_t got = fread(hdr, 1, sizeof hdr, f.get());
        IndexFileHeader h;
        std::string err;
        if (!index_header_check(hdr, got, (uint64_t)st.st_size, h, err)) { fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str()); return nullptr; }
        std::unique_ptr<Index> ix(Index::create(ctx->engine(), (int)h.dim, (int)h.dtype, err));
        if (!ix || !ix->load_rows(f.get(), h, err)) { fprintf(stderr, "%s: '%s': %s\n", me, path, err.c_str()); return nullptr; }
        std::unique_ptr<bert_hip_index> out(new bert_hip_index);
        out->ctx = ctx;
        out->ix = std::move(ix);
        ctx->indexes.push_back(out.get());
        return out.release();
    }, (bert_hip_index *)nullptr);
}

int32_t bert_hip_index_search_texts(struct bert_hip_index *ix, int32_t n_threads, int32_t n_queries, const char **texts, int32_t k,
                                    int32_t *ids, float *scores) {
    const char *me = "bert_hip_index_search_texts";
    return index_call(me, ix, [&](bert_ctx *ctx, Index &x, std::string &err) -> int32_t {
        if (!dim_ok(me, ctx, x)) return -2;
        if (k < 1 || k > Index::MAX_K) { fprintf(stderr, "%s: k must be 1 .. 256\n", me); return -2; }
        if (n_queries < 0 || (n_queries > 0 && (!texts || !ids || !scores))) { fprintf(stderr, "%s: n_queries >= 0 and texts / outputs required\n", me); return -2; }
        if (n_queries == 0) return 0;
        bool ok;
        // (results land in a buffer of our own: the caller's outputs stay untouched on an error)
        std::vector<int32_t> hid((size_t)n_queries * k);
        std::vector<float> hsc((size_t)n_queries * k);
        if (ctx->engines.size() > 1) {
            std::vector<float> emb;
            ok = encode_host(ctx, n_threads, n_queries, texts, emb, err) && x.search_to_host(n_queries, emb.data(), false, k, hid.data(), hsc.data(), err) == 0;
        } else {
            ok = encode_groups_device(ctx, x, n_threads, n_queries, texts, [&](int32_t i0, int32_t c, const float *d) {
                return x.search_to_host(c, d, true, k, hid.data() + (size_t)i0 * k, hsc.data() + (size_t)i0 * k, err) == 0;
            }, err);
        }
        if (!ok) {
            if (err.empty()) err = "device error";
            return -3;
        }
        memcpy(ids, hid.data(), hid.size() * 4);
        memcpy(scores, hsc.data(), hsc.size() * 4);
        return 0;
    });
}

}  // extern "C"
