// tokens_api.cpp — the C ABI of bert_hip.h's "token rows and late interaction" section: per-token final states out of the forward
// pass (Engine::eval_packed_device's token-rows destination; misc_kernels.hip token_rows_kernel) and MaxSim scoring of two sets of
// token rows (maxsim.hip).  Host-side glue only.
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

// the packed batch of a host call: 1 = evaluate, else the entry's result (bert_api.cpp's rules: -1 no device, 0 nothing to do, -2 after a
// line on stderr for a sentence that cannot be evaluated)
int32_t token_batch_status(const bert_ctx *ctx, const char *me, const bert_vocab_id *tokens, const int32_t *cu, int32_t n_sentences) {
    if (!ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
    if (n_sentences <= 0) return 0;
    if (!tokens || !cu) { fprintf(stderr, "%s: tokens and cu_seqlens required\n", me); return -2; }
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

// H, the counts and the pointers both forms of MaxSim check
bool maxsim_shape_ok(const char *me, const void *q, const void *qcu, int32_t n_q, const void *d, const void *dcu, int32_t n_d, int32_t H,
                     const void *pairs, int32_t n_pairs, const void *scores) {
    if (H < 8 || H > MAXSIM_MAX_H || H % 8) { fprintf(stderr, "%s: H = %d (a multiple of 8 in [8, %d] required)\n", me, H, MAXSIM_MAX_H); return false; }
    if (n_q < 1 || n_d < 1 || !q || !qcu || !d || !dcu || !scores || (pairs && n_pairs < 1) || (!pairs && (long long)n_q * n_d > INT_MAX)) {
        fprintf(stderr, "%s: rows, cumulative lengths and scores required, n_q, n_d >= 1, n_pairs >= 1 with a pair list, n_q n_d < 2^31 without\n", me);
        return false;
    }
    return true;
}

// cu: n + 1 strictly ascending entries from 0 on (no empty sentence)
bool cu_ok(const int32_t *cu, int32_t n) {
    bool ok = cu[0] >= 0;
    for (int32_t i = 0; ok && i < n; ++i) ok = cu[i + 1] > cu[i];
    return ok;
}

}  // namespace

extern "C" {

int32_t bert_hip_eval_packed_tokens_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens, int32_t n_sentences,
                                           int32_t n_tokens_total, int32_t max_len, int32_t flags, void *d_rows, float *d_embeddings, void *stream) {
    const char *me = "bert_hip_eval_packed_tokens_device";
    return guarded(me, [&]() -> int32_t {
        if (!ctx || !ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
        if (max_len > ctx->hp.n_max_tokens) { fprintf(stderr, "Too many tokens, maximum is %d\n", ctx->hp.n_max_tokens); return -2; }
        if (max_len <= 0 || n_tokens_total > (long long)n_sentences * max_len) {
            fprintf(stderr, "%s: max_len = %d cannot hold %d tokens in %d sentences\n", me, max_len, n_tokens_total, n_sentences);
            return -2;
        }
        // (launch_token_rows: a workgroup of 256 threads per four tokens in one launch, which holds fewer than 2^32 threads)
        if (n_tokens_total > TOKEN_ROWS_MAX_T) { fprintf(stderr, "%s: more than 2^25 tokens in one call\n", me); return -2; }
        if ((flags & ~3) || (n_sentences > 0 && n_tokens_total > 0 && (!d_rows || !d_tokens || !d_cu_seqlens))) {
            fprintf(stderr, "%s: flags 0 .. 3 and tokens, cu_seqlens, rows required\n", me);
            return -2;
        }
        std::string err;
        if (ctx->engine()->eval_packed_device(d_tokens, d_cu_seqlens, n_sentences, n_tokens_total, max_len, d_embeddings, (hipStream_t)stream, nullptr, err,
                                              nullptr, 0, 0, -1, d_rows, flags) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_eval_packed_tokens(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences, int32_t flags,
                                    float *rows, float *embeddings) {
    const char *me = "bert_hip_eval_packed_tokens";
    return guarded(me, [&]() -> int32_t {
        if (!ctx) return -1;
        const int32_t st = token_batch_status(ctx, me, tokens, cu_seqlens, n_sentences);
        if (st != 1) return st;
        if ((flags & ~1) || !rows) { fprintf(stderr, "%s: flags 0 | 1 and rows required\n", me); return -2; }
        std::string err;
        if (ctx->engine()->eval_packed_tokens_host(tokens, cu_seqlens, n_sentences, flags, rows, embeddings, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return 0;
    }, (int32_t)-4);
}

int64_t bert_hip_encode_tokens_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, int32_t flags, int32_t *cu_out,
                                     float *rows, int64_t cap_rows) {
    const char *me = "bert_hip_encode_tokens_batch";
    return guarded(me, [&]() -> int64_t {
        if (!ctx || !ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
        if (n_inputs < 0 || (n_inputs > 0 && (!texts || !cu_out)) || (flags & ~1)) { fprintf(stderr, "%s: texts, cu_out and flags 0 | 1 required\n", me); return -2; }
        if (cu_out) cu_out[0] = 0;
        if (n_inputs == 0) return 0;
        const size_t N = ctx->hp.n_max_tokens;
        std::vector<int32_t> ids((size_t)n_inputs * N), counts(n_inputs);
        ctx->texts.tokenize_many(n_threads, n_inputs, texts, ids.data(), counts.data());
        long long total = 0;
        for (int32_t i = 0; i < n_inputs; ++i) {
            total += counts[i];
            if (total > INT_MAX) { fprintf(stderr, "%s: more than 2^31 - 1 tokens in one call\n", me); return -2; }
            cu_out[i + 1] = (int32_t)total;
        }
        if (!rows || cap_rows < total) return total;
        std::vector<int32_t> packed((size_t)total);
        for (int32_t i = 0; i < n_inputs; ++i) memcpy(packed.data() + cu_out[i], ids.data() + (size_t)i * N, sizeof(int32_t) * (size_t)counts[i]);
        std::string err;
        if (ctx->engine()->eval_packed_tokens_host(packed.data(), cu_out, n_inputs, flags, rows, nullptr, err) != 0) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -3;
        }
        return total;
    }, (int64_t)-4);
}

int32_t bert_hip_maxsim_device(struct bert_ctx *ctx, const void *d_q, const int32_t *d_qcu, int32_t n_q, const void *d_d, const int32_t *d_dcu, int32_t n_d,
                               int32_t H, const int32_t *d_pairs, int32_t n_pairs, int32_t mode, float *d_scores, void *stream) {
    const char *me = "bert_hip_maxsim_device";
    return guarded(me, [&]() -> int32_t {
        if (!ctx || !ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
        if (!maxsim_shape_ok(me, d_q, d_qcu, n_q, d_d, d_dcu, n_d, H, d_pairs, n_pairs, d_scores)) return -2;
        if (((uintptr_t)d_q | (uintptr_t)d_d) & 15) { fprintf(stderr, "%s: the rows must be 16-byte aligned\n", me); return -2; }
        Engine *e = ctx->engine();
        if (hipSetDevice(e->device()) != hipSuccess) { fprintf(stderr, "%s: hipSetDevice failed\n", me); return -3; }
        MaxsimArgs a{(const half_t *)d_q, (const half_t *)d_d, d_qcu, d_dcu, d_pairs, d_scores, n_q, n_d, H, d_pairs ? n_pairs : 0, mode, 0};
        const hipStream_t s = (hipStream_t)stream;
        // (no workspace, so no event: the call only asks whether s may take the launch — not a capturing stream while the context profiles)
        Engine::StreamOp op;
        std::string err;
        if (!e->op_begin(s, nullptr, op, err)) { fprintf(stderr, "%s: %s\n", me, err.c_str()); return -3; }
        // (flops: unknown without the lengths, which live on the device)
        // (more than MAXSIM_LAUNCH_PAIRS pairs go in several launches, which the profiler does not take as a sample: profiler.h)
        e->timed_launch("maxsim", 0.0, s, [&] { launch_maxsim(a, s, e->options().maxsim_launch_pairs); });
        if (hipGetLastError() != hipSuccess) { fprintf(stderr, "%s: the launch failed\n", me); return -3; }
        return 0;
    }, (int32_t)-4);
}

int32_t bert_hip_maxsim(struct bert_ctx *ctx, const float *q, const int32_t *qcu, int32_t n_q, const float *d, const int32_t *dcu, int32_t n_d, int32_t H,
                        const int32_t *pairs, int32_t n_pairs, int32_t mode, float *scores) {
    const char *me = "bert_hip_maxsim";
    return guarded(me, [&]() -> int32_t {
        if (!ctx || !ctx->engine()) { fprintf(stderr, "%s: tokenizer-only context\n", me); return -1; }
        if (!maxsim_shape_ok(me, q, qcu, n_q, d, dcu, n_d, H, pairs, n_pairs, scores)) return -2;
        bool ok = cu_ok(qcu, n_q) && cu_ok(dcu, n_d);
        for (int32_t i = 0; ok && pairs && i < n_pairs; ++i) ok = pairs[2 * i] >= 0 && pairs[2 * i] < n_q && pairs[2 * i + 1] >= 0 && pairs[2 * i + 1] < n_d;
        if (!ok) {
            fprintf(stderr, "%s: cumulative lengths must ascend strictly from an entry >= 0 and every pair lie in [0, n_q) x [0, n_d)\n", me);
            return -2;
        }
        Engine *e = ctx->engine();
        const hipStream_t s = e->stream();
        std::string err;
        auto fail = [&](const char *what) { fprintf(stderr, "%s: %s\n", me, what ? what : err.c_str()); (void)hipStreamSynchronize(s); return (int32_t)-3; };
        if (hipSetDevice(e->device()) != hipSuccess) return fail("hipSetDevice failed");
        const size_t nqt = (size_t)qcu[n_q], ndt = (size_t)dcu[n_d], n_out = pairs ? (size_t)n_pairs : (size_t)n_q * n_d;
        // (launch_f32_to_f16 rounds a set in one launch of a thread per value)
        if (nqt * H > F32_TO_F16_MAX_N || ndt * H > F32_TO_F16_MAX_N) { fprintf(stderr, "%s: a set of more than 2^31 values (tokens x H)\n", me); return -2; }
        DevBuf q32, d32, q16, d16, cu, pr, out;
        // one upload for qcu | dcu | pairs
        std::vector<int32_t> in(qcu, qcu + n_q + 1);
        in.insert(in.end(), dcu, dcu + n_d + 1);
        if (pairs) in.insert(in.end(), pairs, pairs + 2 * (size_t)n_pairs);
        if (!q32.upload(q, nqt * H * 4, err) || !d32.upload(d, ndt * H * 4, err) || !q16.alloc(nqt * H * 2, err) || !d16.alloc(ndt * H * 2, err) ||
            !cu.upload(in, err) || !out.alloc(n_out * 4, err))
            return fail(nullptr);
        launch_f32_to_f16(q32.as<float>(), q16.as<half_t>(), nqt * H, s);
        launch_f32_to_f16(d32.as<float>(), d16.as<half_t>(), ndt * H, s);
        const int32_t *d_cu = cu.as<int32_t>();
        const int32_t r = bert_hip_maxsim_device(ctx, q16.p, d_cu, n_q, d16.p, d_cu + n_q + 1, n_d, H, pairs ? d_cu + n_q + 1 + n_d + 1 : nullptr, n_pairs, mode,
                                                 out.as<float>(), s);
        if (r != 0) { (void)hipStreamSynchronize(s); return r; }
        if (hipMemcpyAsync(scores, out.p, n_out * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("the copy of the scores failed");
        return 0;
    }, (int32_t)-4);
}

}  // extern "C"
