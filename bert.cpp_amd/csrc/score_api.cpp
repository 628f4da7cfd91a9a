// score_api.cpp — the C ABI of bert_hip.h's "sentence pairs and scores" section: passes with token types (Engine::eval_packed_device's
// first_len; the TYPED embedding kernels of misc_kernels.hip / f32_route.hip), the classification head behind them (cls_head.hip) and the
// pair tokenization that goes with a cross-encoder.  Host-side glue only.  On a context of several GPUs everything here runs on the first.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bert.h"
#include "../../include/bert_hip.h"
#include "abi.h"

using namespace bert_hip;

namespace {

// the packed, typed batch of a host call: 1 = evaluate, else the entry's result (-1 no device, -2 after a line on stderr: no head where
// one is needed, a sentence that cannot be evaluated or a first_len outside [0, length]; 0 nothing to do)
int32_t typed_batch_status(const bert_ctx *ctx, const char *me, bool need_head, const bert_vocab_id *tokens, const int32_t *cu, const int32_t *first_len,
                           int32_t n_sentences, const void *out) {
    if (!ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
    if (need_head && ctx->engine()->n_labels() <= 0) { fprintf(stderr, "%s: the model file has no classification head (pooler.dense.*, classifier.*)\n", me); return -2; }
    if (n_sentences <= 0) return 0;
    if (!tokens || !cu || !out) { fprintf(stderr, "%s: tokens, cu_seqlens and the output required\n", me); return -2; }
    for (int32_t b = 0; b < n_sentences; ++b) {
        const int32_t n = cu[b + 1] - cu[b];
        if (n > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
        if (n <= 0) { fprintf(stderr, "%s: empty input\n", me); return -2; }
        for (int32_t i = cu[b]; i < cu[b + 1]; ++i)
            if (tokens[i] < 0 || tokens[i] >= ctx->hp.n_vocab) {
                fprintf(stderr, "%s: token id %d out of range [0, %d)\n", me, tokens[i], ctx->hp.n_vocab);
                return -2;
            }
        if (first_len && (first_len[b] < 0 || first_len[b] > n)) {
            fprintf(stderr, "%s: first_len[%d] = %d outside [0, %d]\n", me, b, first_len[b], n);
            return -2;
        }
    }
    return 1;
}

// what opens the device forms: 1 = go on, else the entry's result
int32_t device_call_status(const bert_ctx *ctx, const char *me, bool need_head, int32_t n_sentences, int32_t n_tokens_total, int32_t max_len) {
    if (!ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
    if (need_head && ctx->engine()->n_labels() <= 0) { fprintf(stderr, "%s: the model file has no classification head (pooler.dense.*, classifier.*)\n", me); return -2; }
    if (max_len > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
    if (max_len <= 0 || n_tokens_total > (long long)n_sentences * max_len) {
        fprintf(stderr, "%s: max_len = %d cannot hold %d tokens in %d sentences\n", me, max_len, n_tokens_total, n_sentences);
        return -2;
    }
    return 1;
}

// a's ids [CLS] .. [SEP] (la >= 2) and b's (lb >= 2; its [CLS] is dropped) as one sentence of at most n_max ids (n_max >= 4): when the two
// exceed it, a is cut to at most n_max / 2 ids and b to the remainder, each cut keeping its [SEP] last.  Returns the count; *first_len = a's.
int32_t join_pair(const int32_t *a, int32_t la, const int32_t *b, int32_t lb, int32_t n_max, int32_t *out, int32_t *first_len) {
    ++b; --lb;
    int32_t na = la, nb = lb;
    if (na + nb > n_max) {
        na = std::min(na, n_max / 2);
        nb = std::min(nb, n_max - na);
    }
    memcpy(out, a, sizeof(int32_t) * (size_t)na);
    out[na - 1] = a[la - 1];
    memcpy(out + na, b, sizeof(int32_t) * (size_t)nb);
    out[na + nb - 1] = b[lb - 1];
    *first_len = na;
    return na + nb;
}

}  // namespace

extern "C" {

int32_t bert_hip_relative_attention(struct bert_ctx *ctx) { return ctx ? (ctx->rel_bias ? 1 : 0) : -1; }
int32_t bert_hip_n_labels(struct bert_ctx *ctx) { return ctx && ctx->engine() ? ctx->engine()->n_labels() : 0; }

int32_t bert_hip_tokenize_pair(struct bert_ctx *ctx, const char *text_a, const char *text_b, bert_vocab_id *tokens, int32_t *n_tokens,
                               int32_t *first_len, int32_t n_max_tokens) {
    const char *me = "bert_hip_tokenize_pair";
    return guarded(me, [&]() -> int32_t {
        if (!ctx || !text_a || !text_b || !tokens || !n_tokens || !first_len || n_max_tokens < 4) {
            fprintf(stderr, "%s: two texts, tokens, n_tokens, first_len and n_max_tokens >= 4 required\n", me);
            return -2;
        }
        std::vector<int32_t> a((size_t)n_max_tokens), b((size_t)n_max_tokens);
        int32_t la = 0, lb = 0;
        ctx->tok.tokenize(text_a, a.data(), &la, n_max_tokens);
        ctx->tok.tokenize(text_b, b.data(), &lb, n_max_tokens);
        *n_tokens = join_pair(a.data(), la, b.data(), lb, n_max_tokens, tokens, first_len);
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_typed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, const int32_t *first_len,
                                   int32_t n_sentences, float *embeddings) {
    const char *me = "bert_hip_eval_packed_typed";
    return guarded(me, [&]() -> int32_t {
        if (!ctx) return -1;
        const int32_t st = typed_batch_status(ctx, me, false, tokens, cu_seqlens, first_len, n_sentences, embeddings);
        if (st != 1) return st;
        std::string err;
        if (ctx->engine()->eval_packed_typed_host(tokens, cu_seqlens, first_len, n_sentences, false, 0, embeddings, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_typed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens, const int32_t *d_first_len,
                                          int32_t n_sentences, int32_t n_tokens_total, int32_t max_len, float *d_embeddings, void *stream) {
    const char *me = "bert_hip_eval_packed_typed_device";
    return guarded(me, [&]() -> int32_t {
        if (!ctx) return -1;
        const int32_t st = device_call_status(ctx, me, false, n_sentences, n_tokens_total, max_len);
        if (st != 1) return st;
        std::string err;
        if (ctx->engine()->eval_packed_device(d_tokens, d_cu_seqlens, n_sentences, n_tokens_total, max_len, d_embeddings, (hipStream_t)stream, nullptr, err,
                                              nullptr, 0, 0, -1, nullptr, 0, d_first_len) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_score_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, const int32_t *first_len,
                              int32_t n_sentences, int32_t flags, float *scores) {
    const char *me = "bert_hip_score_packed";
    return guarded(me, [&]() -> int32_t {
        if (!ctx) return -1;
        const int32_t st = typed_batch_status(ctx, me, true, tokens, cu_seqlens, first_len, n_sentences, scores);
        if (st != 1) return st;
        if (flags & ~1) { fprintf(stderr, "%s: flags 0 | 1\n", me); return -2; }
        std::string err;
        if (ctx->engine()->eval_packed_typed_host(tokens, cu_seqlens, first_len, n_sentences, true, flags, scores, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_score_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens, const int32_t *d_first_len,
                                     int32_t n_sentences, int32_t n_tokens_total, int32_t max_len, int32_t flags, float *d_scores, void *stream) {
    const char *me = "bert_hip_score_packed_device";
    return guarded(me, [&]() -> int32_t {
        if (!ctx) return -1;
        const int32_t st = device_call_status(ctx, me, true, n_sentences, n_tokens_total, max_len);
        if (st != 1) return st;
        if ((flags & ~1) || (n_sentences > 0 && n_tokens_total > 0 && (!d_tokens || !d_cu_seqlens || !d_scores))) {
            fprintf(stderr, "%s: flags 0 | 1 and tokens, cu_seqlens, scores required\n", me);
            return -2;
        }
        std::string err;
        if (ctx->engine()->score_packed_device(d_tokens, d_cu_seqlens, d_first_len, n_sentences, n_tokens_total, max_len, flags, d_scores, (hipStream_t)stream, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_score_pairs(struct bert_ctx *ctx, int32_t n_threads, int32_t n_pairs, const char **texts_a, const char **texts_b, int32_t flags,
                             float *scores) {
    const char *me = "bert_hip_score_pairs";
    return guarded(me, [&]() -> int32_t {
        if (!ctx || !ctx->engine()) { fprintf(stderr, "%s: this context has no device weights (tokenizer-only)\n", me); return -1; }
        const int32_t NL = ctx->engine()->n_labels();
        if (NL <= 0) { fprintf(stderr, "%s: the model file has no classification head (pooler.dense.*, classifier.*)\n", me); return -2; }
        if (ctx->rel_bias) {
            fprintf(stderr, "%s: the model has a relative position bias (MPNet): its pair layout, <s> a </s></s> b </s>, is not built here; pack the ids and call bert_hip_score_packed\n", me);
            return -2;
        }
        if (n_pairs <= 0) return 0;
        if (!texts_a || !texts_b || !scores || (flags & ~1)) { fprintf(stderr, "%s: texts, scores and flags 0 | 1 required\n", me); return -2; }
        const int32_t N = ctx->hp.n_max_tokens;
        if (N < 4) { fprintf(stderr, "%s: the model's n_max_tokens = %d cannot hold a pair\n", me, N); return -2; }
        // groups of at most 4096 pairs: the id buffers stay bounded for any n_pairs
        constexpr int32_t GROUP = 4096;
        std::vector<int32_t> ids_a, ids_b, cnt_a, cnt_b, packed, cu, fl;
        std::string err;
        for (int32_t i0 = 0; i0 < n_pairs; i0 += GROUP) {
            const int32_t n = std::min(GROUP, n_pairs - i0);
            ids_a.resize((size_t)n * N); ids_b.resize((size_t)n * N); cnt_a.resize(n); cnt_b.resize(n);
            ctx->texts.tokenize_many(n_threads, n, texts_a + i0, ids_a.data(), cnt_a.data());
            ctx->texts.tokenize_many(n_threads, n, texts_b + i0, ids_b.data(), cnt_b.data());
            packed.resize((size_t)n * N); cu.assign((size_t)n + 1, 0); fl.resize(n);
            for (int32_t i = 0; i < n; ++i)
                cu[i + 1] = cu[i] + join_pair(ids_a.data() + (size_t)i * N, cnt_a[i], ids_b.data() + (size_t)i * N, cnt_b[i], N, packed.data() + cu[i], &fl[i]);
            if (ctx->engine()->eval_packed_typed_host(packed.data(), cu.data(), fl.data(), n, true, flags, scores + (size_t)i0 * NL, err) != 0) {
                fprintf(stderr, "%s: %s\n", me, err.c_str());
                return i0 ? i0 : -3;
            }
        }
        return n_pairs;
    }, (int32_t)-4);
}

}  // extern "C"
