// sparse_api.cpp — the C ABI of bert_hip.h's "learned sparse embeddings" section: a pass, the MLM transform and the vocabulary launch behind
// it (Engine::sparse_packed_device; sparse_vocab.hip), dense or as top-k terms.  Host-side glue only.  On a context of several GPUs
// everything here runs on the first.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bert.h"
#include "../../include/bert_hip.h"
#include "abi.h"

using namespace bert_hip;

namespace {

const char *const kNoHead = "the model file has no MLM head (cls.predictions.*)";

// what every entry checks first: 1 = go on, else the entry's result (-1 no device; -2 after a line on stderr: no head, or a k outside
// [1, 256] where one is taken)
int32_t head_status(const bert_ctx *ctx, const char *me, bool topk, int32_t k) {
    if (!ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
    if (!ctx->engine()->has_mlm_head()) { fprintf(stderr, "%s: %s\n", me, kNoHead); return -2; }
    if (topk && (k < 1 || k > SPARSE_MAX_K)) { fprintf(stderr, "%s: k = %d outside 1 .. %d\n", me, k, SPARSE_MAX_K); return -2; }
    return 1;
}

// the packed batch of a host call: 1 = evaluate, 0 nothing to do, -2 after a line on stderr
int32_t batch_status(const bert_ctx *ctx, const char *me, const bert_vocab_id *tokens, const int32_t *cu, int32_t n_sentences, bool outputs) {
    if (n_sentences <= 0) return 0;
    if (!tokens || !cu || !outputs) { fprintf(stderr, "%s: tokens, cu_seqlens and the outputs required\n", me); return -2; }
    for (int32_t b = 0; b < n_sentences; ++b) {
        const int32_t n = cu[b + 1] - cu[b];
        if (n > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
        if (n <= 0) { fprintf(stderr, "%s: empty input\n", me); return -2; }
        for (int32_t i = cu[b]; i < cu[b + 1]; ++i)
            if (tokens[i] < 0 || tokens[i] >= ctx->hp.n_vocab) {
                fprintf(stderr, "%s: token id %d out of range [0, %d)\n", me, tokens[i], ctx->hp.n_vocab);
                return -2;
            }
    }
    return 1;
}

int32_t host_call(bert_ctx *ctx, const char *me, const bert_vocab_id *tokens, const int32_t *cu, int32_t n_sentences, bool topk, int32_t k, int32_t *ids,
                  float *weights) {
    if (!ctx) return -1;
    int32_t st = head_status(ctx, me, topk, k);
    if (st != 1) return st;
    st = batch_status(ctx, me, tokens, cu, n_sentences, weights && (!topk || ids));
    if (st != 1) return st;
    std::string err;
    if (ctx->engine()->sparse_packed_host(tokens, cu, n_sentences, topk ? k : 0, ids, weights, err) != 0) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -3;
    }
    return 0;
}

int32_t device_call(bert_ctx *ctx, const char *me, const bert_vocab_id *d_tokens, const int32_t *d_cu, int32_t n_sentences, int32_t n_tokens_total,
                    int32_t max_len, bool topk, int32_t k, int32_t *d_ids, float *d_weights, void *stream) {
    if (!ctx) return -1;
    const int32_t st = head_status(ctx, me, topk, k);
    if (st != 1) return st;
    if (n_sentences <= 0 || n_tokens_total <= 0) return 0;
    if (max_len > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
    if (max_len <= 0 || n_tokens_total > (long long)n_sentences * max_len) {
        fprintf(stderr, "%s: max_len = %d cannot hold %d tokens in %d sentences\n", me, max_len, n_tokens_total, n_sentences);
        return -2;
    }
    if (!d_tokens || !d_cu || !d_weights || (topk && !d_ids)) { fprintf(stderr, "%s: tokens, cu_seqlens and the outputs required\n", me); return -2; }
    std::string err;
    if (ctx->engine()->sparse_packed_device(d_tokens, d_cu, n_sentences, n_tokens_total, max_len, topk ? k : 0, d_ids, d_weights, (hipStream_t)stream, err) != 0) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -3;
    }
    return 0;
}

}  // namespace

extern "C" {

int32_t bert_hip_has_mlm_head(struct bert_ctx *ctx) { return ctx && ctx->engine() && ctx->engine()->has_mlm_head() ? 1 : 0; }

int32_t bert_hip_sparse_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences, float *weights) {
    const char *me = "bert_hip_sparse_packed";
    return guarded(me, [&]() -> int32_t { return host_call(ctx, me, tokens, cu_seqlens, n_sentences, false, 0, nullptr, weights); }, (int32_t)-4);
}

int32_t bert_hip_sparse_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens, int32_t n_sentences,
                                      int32_t n_tokens_total, int32_t max_len, float *d_weights, void *stream) {
    const char *me = "bert_hip_sparse_packed_device";
    return guarded(me, [&]() -> int32_t {
        return device_call(ctx, me, d_tokens, d_cu_seqlens, n_sentences, n_tokens_total, max_len, false, 0, nullptr, d_weights, stream);
    }, (int32_t)-4);
}

int32_t bert_hip_sparse_topk_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences, int32_t k,
                                    int32_t *ids, float *weights) {
    const char *me = "bert_hip_sparse_topk_packed";
    return guarded(me, [&]() -> int32_t { return host_call(ctx, me, tokens, cu_seqlens, n_sentences, true, k, ids, weights); }, (int32_t)-4);
}

int32_t bert_hip_sparse_topk_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens, int32_t n_sentences,
                                           int32_t n_tokens_total, int32_t max_len, int32_t k, int32_t *d_ids, float *d_weights, void *stream) {
    const char *me = "bert_hip_sparse_topk_packed_device";
    return guarded(me, [&]() -> int32_t {
        return device_call(ctx, me, d_tokens, d_cu_seqlens, n_sentences, n_tokens_total, max_len, true, k, d_ids, d_weights, stream);
    }, (int32_t)-4);
}

int32_t bert_hip_encode_sparse_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, int32_t k, int32_t *ids, float *weights) {
    const char *me = "bert_hip_encode_sparse_batch";
    return guarded(me, [&]() -> int32_t {
        if (!ctx) return -1;
        const int32_t st = head_status(ctx, me, true, k);
        if (st != 1) return st;
        if (n <= 0) return 0;
        if (!texts || !ids || !weights) { fprintf(stderr, "%s: texts, ids and weights required\n", me); return -2; }
        const int32_t N = ctx->hp.n_max_tokens;
        // groups of at most 4096 texts: the id buffers stay bounded for any n
        constexpr int32_t GROUP = 4096;
        std::vector<int32_t> tok, cnt, packed, cu;
        std::string err;
        for (int32_t i0 = 0; i0 < n; i0 += GROUP) {
            const int32_t m = std::min(GROUP, n - i0);
            tok.resize((size_t)m * N); cnt.resize(m);
            ctx->texts.tokenize_many(n_threads, m, texts + i0, tok.data(), cnt.data());
            packed.resize((size_t)m * N); cu.assign((size_t)m + 1, 0);
            for (int32_t i = 0; i < m; ++i) {
                memcpy(packed.data() + cu[i], tok.data() + (size_t)i * N, sizeof(int32_t) * (size_t)cnt[i]);
                cu[i + 1] = cu[i] + cnt[i];
            }
            if (ctx->engine()->sparse_packed_host(packed.data(), cu.data(), m, k, ids + (size_t)i0 * k, weights + (size_t)i0 * k, err) != 0) {
                fprintf(stderr, "%s: %s\n", me, err.c_str());
                return i0 ? i0 : -3;
            }
        }
        return n;
    }, (int32_t)-4);
}

}  // extern "C"
