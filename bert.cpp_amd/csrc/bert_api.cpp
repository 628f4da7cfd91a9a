// bert_api.cpp — the C ABI of libbert.so: bert.h (the reference's API, symbol for symbol) and the
// bert_hip.h extensions but for the embedding index (index_api.cpp).  Host-side glue only; every FLOP of bert_eval runs in the
// HIP kernels.  The context and its loading are context.h's, the text pipeline text_batch.h's, the multi-device evaluation and
// the gather gather.h's.
//
// Reference behaviour mirrored here (reference file:line):
//   bert_load_from_file  bert.cpp:331-694    bert_free          bert.cpp:715-718
//   bert_tokenize        bert.cpp:252-325    bert_eval          bert.cpp:720-728
//   bert_eval_batch      bert.cpp:730-941    bert_encode        bert.cpp:943-950
//   bert_encode_batch    bert.cpp:952-1022   accessors          bert.cpp:111-134
//   bert_params_parse    bert.cpp:140-193
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/bert.h"
#include "../../include/bert_hip.h"
#include "abi.h"

using namespace bert_hip;

namespace {

// Validates sentence b; returns false (after the reference's stderr message) if it cannot be evaluated.
bool sentence_ok(const bert_ctx *ctx, const bert_vocab_id *toks, int32_t n) {
    if (n > ctx->hp.n_max_tokens) {
        fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens);   // reference bert.cpp:765-769
        return false;
    }
    if (n <= 0 || !toks) {
        fprintf(stderr, "bert_eval_batch: empty input\n");
        return false;
    }
    for (int32_t i = 0; i < n; ++i)
        if (toks[i] < 0 || toks[i] >= ctx->hp.n_vocab) {
            fprintf(stderr, "bert_eval_batch: token id %d out of range [0, %d)\n", toks[i], ctx->hp.n_vocab);
            return false;
        }
    return true;
}

// What opens the packed evaluation entries: 1 if there is a batch to evaluate, else the entry's result (-1 for a context
// without a device, 0 for no sentences, -2 after the message of the first sentence that cannot be evaluated).
int32_t packed_batch_status(const bert_ctx *ctx, const char *me, const bert_vocab_id *tokens, const int32_t *cu, int32_t n_sentences) {
    if (!ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
    if (n_sentences <= 0) return 0;
    for (int32_t b = 0; b < n_sentences; ++b)
        if (!sentence_ok(ctx, tokens + cu[b], cu[b + 1] - cu[b])) return -2;
    return 1;
}

// B validated sentences, packed, into the caller's rows: B, or -1 on a device error
int32_t eval_packed_rows(bert_ctx *ctx, const bert_vocab_id *packed, const int32_t *cu, int32_t B, float *const *batch_embeddings) {
    const int H = ctx->hp.n_embd;
    // the caller's rows are usually the rows of ONE matrix (NumPy rows through ctypes: reference examples/sample_dylib.py:50-51):
    // then the engine writes them in place; scattered rows go through a matrix of our own.  (A device error half way through a
    // call of several chunks leaves the rows of the finished chunks written in the first case, nothing in the second.)
    bool rows_of_one_matrix = true;
    for (int32_t b = 1; b < B && rows_of_one_matrix; ++b) rows_of_one_matrix = batch_embeddings[b] == batch_embeddings[0] + (size_t)b * H;
    std::vector<float> out(rows_of_one_matrix ? 0 : (size_t)B * H);
    std::string err;
    if (eval_packed_all_devices(ctx->engines, ctx->workers.get(), packed, cu, B, rows_of_one_matrix ? batch_embeddings[0] : out.data(), err) != 0) {
        fprintf(stderr, "bert_eval_batch: %s\n", err.c_str());
        return -1;
    }
    if (!rows_of_one_matrix)
        for (int32_t b = 0; b < B; ++b) memcpy(batch_embeddings[b], out.data() + (size_t)b * H, sizeof(float) * H);
    return B;
}

// returns the number of sentences evaluated (stops in front of the first one it cannot handle), -1 on a device error
int32_t eval_batch_impl(bert_ctx *ctx, int32_t n_batch_size, bert_vocab_id *const *batch_tokens, const int32_t *n_tokens,
                        float *const *batch_embeddings) {
    if (!ctx->engine()) { fprintf(stderr, "bert_eval_batch: this context has no device weights (tokenizer-only)\n"); return -1; }
    if (n_batch_size <= 0) return 0;
    if (ctx->inject_bad_alloc) throw std::bad_alloc();           // test knob: the path an exhausted host takes
    // The reference evaluates sentences in order and stops at the first one it cannot handle,
    // leaving later outputs untouched; keep that observable behaviour.
    int32_t B = 0;
    for (; B < n_batch_size; ++B)
        if (!sentence_ok(ctx, batch_tokens[B], n_tokens[B])) break;
    if (B == 0) return 0;
    std::vector<int32_t> cu(B + 1, 0);
    for (int32_t b = 0; b < B; ++b) cu[b + 1] = cu[b] + n_tokens[b];
    std::vector<int32_t> packed((size_t)cu[B]);
    for (int32_t b = 0; b < B; ++b) memcpy(packed.data() + cu[b], batch_tokens[b], sizeof(int32_t) * n_tokens[b]);
    return eval_packed_rows(ctx, packed.data(), cu.data(), B, batch_embeddings);
}

}  // namespace

// Tokenized on n_threads host threads (at 10^6 sentences/s on the GPU the tokenizer is the stage in front of the path that has
// to keep up) and evaluated as packed device batches, group by group (text_batch.h).
int32_t bert_hip::encode_batch_impl(bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, float **embeddings) {
    if (n_inputs <= 0) return 0;
    if (!ctx->engine()) { fprintf(stderr, "bert_encode_batch: this context has no device weights (tokenizer-only)\n"); return -1; }
    if (ctx->inject_bad_alloc) throw std::bad_alloc();           // test knob: the path an exhausted host takes
    return ctx->texts.encode_groups(n_threads, n_inputs, texts, [&](const TokenGroup &g, int32_t i0) {
        return eval_packed_rows(ctx, g.packed.get(), g.cu.data(), g.n_ok, embeddings + i0);
    });
}

// window and stride as bert_hip_plan_windows takes them, for this context's model (-2 after a line on stderr otherwise)
bool bert_hip::long_args_ok(const char *me, const bert_ctx *ctx, int32_t window, int32_t stride) {
    const bool ok = window >= 3 && window <= ctx->hp.n_max_tokens && stride >= 1 && stride <= window - 2;
    if (!ok) fprintf(stderr, "%s: 3 <= window <= %d and 1 <= stride <= window - 2 required (window %d, stride %d)\n", me, ctx->hp.n_max_tokens, window, stride);
    return ok;
}

// Long texts: tokenized without truncation, cut into windows, every window an ordinary sentence, one pooled row per text
// (text_batch.h encode_long_groups; the grouped pooling of gather.h).
int32_t bert_hip::encode_long_batch_impl(bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, int32_t window, int32_t stride,
                                         float **embeddings, int32_t *n_windows) {
    const char *me = "bert_hip_encode_long_batch";
    if (!ctx->engine()) { fprintf(stderr, "%s: this context has no device weights (tokenizer-only)\n", me); return -1; }
    if (!long_args_ok(me, ctx, window, stride)) return -2;
    if (n_inputs <= 0) return 0;
    if (!texts || !embeddings) { fprintf(stderr, "%s: texts and embeddings required\n", me); return -2; }
    const size_t H = ctx->hp.n_embd;
    std::vector<float> out;
    return ctx->texts.encode_long_groups(n_threads, n_inputs, texts, window, stride, n_windows, [&](const LongGroup &g, int32_t i0) -> int32_t {
        const int32_t G = g.n_texts();
        out.resize((size_t)G * H);
        std::string err;
        if (eval_packed_grouped_all_devices(ctx->engines, ctx->workers.get(), g.packed.data(), g.cu.data(), g.n_windows(), g.group_cu.data(), G,
                                            out.data(), nullptr, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -1;
        }
        for (int32_t i = 0; i < G; ++i) memcpy(embeddings[i0 + i], out.data() + (size_t)i * H, sizeof(float) * H);
        return G;
    });
}

extern "C" {

// ------------------------------------------------------------------------------------------------
// bert.h
// ------------------------------------------------------------------------------------------------
bool bert_params_parse(int argc, char **argv, bert_params &params) {
    auto usage = [&]() {
        fprintf(stderr, "usage: %s [options]\n\noptions:\n", argv[0]);
        fprintf(stderr, "  -h, --help            show this help message and exit\n");
        fprintf(stderr, "  -t N, --threads N     accepted for compatibility, ignored by the GPU engine (default: %d)\n", params.n_threads);
        fprintf(stderr, "  -p PROMPT, --prompt PROMPT\n                        text to embed (default: %s)\n", params.prompt);
        fprintf(stderr, "  --port p              port to bind in server mode (default: %d)\n", params.port);
        fprintf(stderr, "  -m FNAME, --model FNAME\n                        model path (default: %s)\n\n", params.model);
    };
    for (int i = 1; i < argc; ++i) {
        const char *arg = argv[i];
        const bool has_value = i + 1 < argc;
        auto is = [&](const char *a, const char *b) { return strcmp(arg, a) == 0 || strcmp(arg, b) == 0; };
        if (is("-t", "--threads") && has_value) params.n_threads = atoi(argv[++i]);
        else if (is("-p", "--prompt") && has_value) params.prompt = argv[++i];
        else if (strcmp(arg, "--port") == 0 && has_value) params.port = atoi(argv[++i]);
        else if (is("-m", "--model") && has_value) params.model = argv[++i];
        else {
            if (!is("-h", "--help")) fprintf(stderr, "error: unknown argument: %s\n", arg);
            usage();
            exit(0);   // the reference exits with status 0 on both paths (bert.cpp:180-189)
        }
    }
    return true;
}

struct bert_ctx *bert_load_from_file(const char *fname) {
    return guarded("bert_load_from_file", [&] { return load_impl(fname, false); }, (bert_ctx *)nullptr);
}

void bert_free(struct bert_ctx *ctx) {
    guarded("bert_free", [&] { delete ctx; });
}

int32_t bert_n_embd(struct bert_ctx *ctx) { return ctx->hp.n_embd; }
int32_t bert_n_max_tokens(struct bert_ctx *ctx) { return ctx->hp.n_max_tokens; }
const char *bert_vocab_id_to_token(struct bert_ctx *ctx, bert_vocab_id id) { return ctx->tok.id_to_token(id); }

void bert_tokenize(struct bert_ctx *ctx, const char *text, bert_vocab_id *tokens, int32_t *n_tokens, int32_t n_max_tokens) {
    guarded("bert_tokenize", [&] { ctx->tok.tokenize(text, tokens, n_tokens, n_max_tokens); });
}

void bert_eval_batch(struct bert_ctx *ctx, int32_t /*n_threads*/, int32_t n_batch_size, bert_vocab_id **batch_tokens,
                     int32_t *n_tokens, float **batch_embeddings) {
    if (!batch_embeddings) return;   // the reference's memory-probe mode (bert.cpp:739); nothing to size here
    guarded("bert_eval_batch", [&] { (void)eval_batch_impl(ctx, n_batch_size, batch_tokens, n_tokens, batch_embeddings); });
}

void bert_eval(struct bert_ctx *ctx, int32_t n_threads, bert_vocab_id *tokens, int32_t n_tokens, float *embeddings) {
    bert_eval_batch(ctx, n_threads, 1, &tokens, &n_tokens, embeddings ? &embeddings : nullptr);
}

void bert_encode_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t /*n_batch_size*/, int32_t n_inputs,
                       const char **texts, float **embeddings) {
    guarded("bert_encode_batch", [&] { (void)encode_batch_impl(ctx, n_threads, n_inputs, texts, embeddings); });
}

void bert_encode(struct bert_ctx *ctx, int32_t n_threads, const char *texts, float *embeddings) {
    bert_encode_batch(ctx, n_threads, 1, 1, &texts, &embeddings);
}

// ------------------------------------------------------------------------------------------------
// bert_hip.h
// ------------------------------------------------------------------------------------------------
struct bert_ctx *bert_hip_load_tokenizer(const char *fname) {
    return guarded("bert_hip_load_tokenizer", [&] { return load_impl(fname, true); }, (bert_ctx *)nullptr);
}

int32_t bert_hip_encode_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, float **embeddings) {
    return guarded("bert_hip_encode_batch", [&] { return encode_batch_impl(ctx, n_threads, n_inputs, texts, embeddings); }, (int32_t)-1);
}

int32_t bert_hip_tokenize_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts,
                                bert_vocab_id *tokens, int32_t *n_tokens) {
    if (!ctx || n_inputs < 0 || (n_inputs > 0 && (!texts || !tokens || !n_tokens))) return -1;
    return guarded("bert_hip_tokenize_batch", [&] { ctx->texts.tokenize_many(n_threads, n_inputs, texts, tokens, n_tokens); return (int32_t)0; }, (int32_t)-1);
}

int32_t bert_hip_n_layer(struct bert_ctx *ctx) { return ctx->hp.n_layer; }
int32_t bert_hip_n_head(struct bert_ctx *ctx) { return ctx->hp.n_head; }
int32_t bert_hip_n_intermediate(struct bert_ctx *ctx) { return ctx->hp.n_intermediate; }
int32_t bert_hip_n_vocab(struct bert_ctx *ctx) { return ctx->hp.n_vocab; }
int32_t bert_hip_ftype(struct bert_ctx *ctx) { return ctx->hp.f16; }
int32_t bert_hip_device(struct bert_ctx *ctx) { return ctx->engine() ? ctx->engine()->device() : -1; }
int32_t bert_hip_n_devices(struct bert_ctx *ctx) { return (int32_t)ctx->engines.size(); }
int32_t bert_hip_pooling(struct bert_ctx *ctx) { return ctx && ctx->engine() ? (int32_t)ctx->engine()->options().pool_cls : -1; }
int32_t bert_hip_normalize(struct bert_ctx *ctx) { return ctx && ctx->engine() ? (int32_t)ctx->engine()->options().normalize : -1; }

int32_t bert_hip_eval_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens,
                             int32_t n_sentences, float *embeddings) {
    return guarded("bert_hip_eval_packed", [&]() -> int32_t {
        const int32_t st = packed_batch_status(ctx, "bert_hip_eval_packed", tokens, cu_seqlens, n_sentences);
        if (st != 1) return st;
        std::string err;
        if (eval_packed_all_devices(ctx->engines, ctx->workers.get(), tokens, cu_seqlens, n_sentences, embeddings, err) != 0) {
            fprintf(stderr, "bert_hip_eval_packed: %s\n", err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_gather(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens,
                                    int32_t n_sentences, float **d_embeddings) {
    return guarded("bert_hip_eval_packed_gather", [&]() -> int32_t {
        const int32_t st = packed_batch_status(ctx, "bert_hip_eval_packed_gather", tokens, cu_seqlens, n_sentences);
        if (st != 1) return st;
        std::string err;
        if (!ctx->gather.run(ctx->engines, ctx->workers.get(), tokens, cu_seqlens, n_sentences, d_embeddings, err)) {
            fprintf(stderr, "bert_hip_eval_packed_gather: %s\n", err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                    int32_t n_sentences, int32_t n_tokens_total, int32_t max_len, float *d_embeddings,
                                    void *stream) {
    return guarded("bert_hip_eval_packed_device", [&]() -> int32_t {
        if (!ctx->engine()) { fprintf(stderr, "bert_hip_eval_packed_device: tokenizer-only context\n"); return -1; }
        if (max_len > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
        if (max_len <= 0 || n_tokens_total > (long long)n_sentences * max_len) {
            fprintf(stderr, "bert_hip_eval_packed_device: max_len = %d cannot hold %d tokens in %d sentences\n", max_len, n_tokens_total, n_sentences);
            return -2;
        }
        std::string err;
        if (ctx->engine()->eval_packed_device(d_tokens, d_cu_seqlens, n_sentences, n_tokens_total, max_len, d_embeddings,
                                              (hipStream_t)stream, nullptr, err) != 0) {
            fprintf(stderr, "bert_hip_eval_packed_device: %s\n", err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_grouped(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences,
                                     const int32_t *group_cu, int32_t n_groups, float *embeddings) {
    const char *me = "bert_hip_eval_packed_grouped";
    return guarded(me, [&]() -> int32_t {
        const int32_t st = packed_batch_status(ctx, me, tokens, cu_seqlens, n_sentences);
        if (st != 1) return st;
        // group_cu before anything is launched: from 0 to n_sentences, strictly increasing (no empty group)
        bool ok = group_cu && embeddings && n_groups >= 1 && n_groups <= n_sentences && group_cu[0] == 0 && group_cu[n_groups] == n_sentences;
        for (int32_t g = 0; ok && g < n_groups; ++g) ok = group_cu[g + 1] > group_cu[g];
        if (!ok) {
            fprintf(stderr, "%s: group_cu must hold n_groups + 1 strictly increasing entries from 0 to n_sentences = %d\n", me, n_sentences);
            return -2;
        }
        std::string err;
        if (eval_packed_grouped_all_devices(ctx->engines, ctx->workers.get(), tokens, cu_seqlens, n_sentences, group_cu, n_groups, embeddings,
                                            nullptr, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_grouped_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens, int32_t n_sentences,
                                            int32_t n_tokens_total, int32_t max_len, const int32_t *d_group_cu, int32_t n_groups,
                                            float *d_embeddings, void *stream) {
    const char *me = "bert_hip_eval_packed_grouped_device";
    return guarded(me, [&]() -> int32_t {
        if (!ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
        if (max_len > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
        if (max_len <= 0 || n_tokens_total > (long long)n_sentences * max_len) {
            fprintf(stderr, "%s: max_len = %d cannot hold %d tokens in %d sentences\n", me, max_len, n_tokens_total, n_sentences);
            return -2;
        }
        if (n_groups < 0 || n_groups > n_sentences || (n_groups > 0 && (!d_group_cu || !d_embeddings))) {
            fprintf(stderr, "%s: 0 <= n_groups <= n_sentences and group_cu / embeddings required\n", me);
            return -2;
        }
        std::string err;
        if (ctx->engine()->eval_packed_grouped_device(d_tokens, d_cu_seqlens, n_sentences, n_tokens_total, max_len, d_group_cu, n_groups,
                                                      d_embeddings, (hipStream_t)stream, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_tokenize_long(struct bert_ctx *ctx, const char *text, bert_vocab_id *tokens, int32_t cap) {
    if (!ctx || !text) return -1;
    return guarded("bert_hip_tokenize_long", [&]() -> int32_t {
        std::vector<int32_t> ids;
        ctx->texts.tokenize_long(text, ids);
        const int32_t n = (int32_t)ids.size();
        if (tokens && cap >= n) memcpy(tokens, ids.data(), sizeof(int32_t) * (size_t)n);
        return n;
    }, (int32_t)-4);
}

int32_t bert_hip_plan_windows(int32_t n_tokens, int32_t window, int32_t stride, int32_t *starts, int32_t cap) {
    return plan_windows(n_tokens, window, stride, starts, cap);
}

int32_t bert_hip_encode_long_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, int32_t window, int32_t stride,
                                   float **embeddings, int32_t *n_windows) {
    if (!ctx) return -1;
    return guarded("bert_hip_encode_long_batch", [&] { return encode_long_batch_impl(ctx, n_threads, n_inputs, texts, window, stride, embeddings, n_windows); },
                   (int32_t)-4);
}

int32_t bert_hip_reserve(struct bert_ctx *ctx, int32_t n_tokens, int32_t n_sentences) {
    return guarded("bert_hip_reserve", [&]() -> int32_t {
        std::string err;
        for (auto &e : ctx->engines)
            if (!e->reserve(n_tokens, n_sentences, err)) { fprintf(stderr, "bert_hip_reserve: %s\n", err.c_str()); return -3; }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_check(struct bert_ctx *ctx) {
    return guarded("bert_hip_check", [&]() -> int32_t {
        int32_t st = 0;
        std::string err;
        for (auto &e : ctx->engines) {
            const int s = e->check(err);
            if (s < 0) { fprintf(stderr, "bert_hip_check: %s\n", err.c_str()); return -3; }
            st |= s;
        }
        if (st) fprintf(stderr, "bert_hip_check: a device batch held a sentence longer than the max_len it was called with (or an empty one): its embeddings are NaN\n");
        return st;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_hidden(struct bert_ctx *ctx, const bert_vocab_id *tokens, int32_t n_tokens, float *hidden,
                             float *embedding) {
    return guarded("bert_hip_eval_hidden", [&]() -> int32_t {
        if (!ctx->engine()) { fprintf(stderr, "bert_hip_eval_hidden: tokenizer-only context\n"); return -1; }
        if (!sentence_ok(ctx, tokens, n_tokens)) return -2;
        std::string err;
        if (ctx->engine()->eval_hidden(tokens, n_tokens, hidden, embedding, err) != 0) {
            fprintf(stderr, "bert_hip_eval_hidden: %s\n", err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

void bert_hip_profile_enable(struct bert_ctx *ctx, int32_t on) {
    guarded("bert_hip_profile_enable", [&] { for (auto &e : ctx->engines) e->profile_enable(on != 0); });
}

int32_t bert_hip_profile_report(struct bert_ctx *ctx, char *buf, int32_t buf_len) {
    return guarded("bert_hip_profile_report", [&]() -> int32_t {
        if (!ctx->engine()) return 0;
        const std::string r = ctx->engine()->profile_report();      // (the first device's kernels)
        for (size_t d = 1; d < ctx->engines.size(); ++d) (void)ctx->engines[d]->profile_report();
        if (buf && buf_len > 0) {
            const size_t n = std::min((size_t)buf_len - 1, r.size());
            memcpy(buf, r.data(), n);
            buf[n] = 0;
        }
        return (int32_t)r.size();
    }, (int32_t)0);
}

void bert_hip_set_option(struct bert_ctx *ctx, const char *key, const char *value) {
    guarded("bert_hip_set_option", [&] {
        if (!key || !value) return;
        if (strcmp(key, "test_inject_bad_alloc") == 0) ctx->inject_bad_alloc = *value == '1';
        else if (strcmp(key, "test_rccl_single") == 0) ctx->gather.rccl_single = *value == '1';
        else if (strcmp(key, "gather_super_tokens") == 0) ctx->gather.super_tokens = std::max(0, atoi(value));
        else
            for (auto &e : ctx->engines) e->set_option(key, value);
    });
}

const char *bert_hip_version(void) { return "bert.cpp_amd 0.5 (gfx950)"; }

}  // extern "C"
