// text_routes.h — how the text entry points of the two indexes (index_api.cpp, sparse_index_api.cpp) and of the hybrid search
// (hybrid_api.cpp) get from texts to device buffers: the embeddings of a group of texts into the embedding index's scratch buffer,
// the chunks of a list of texts into an index's text buffers (text_chunks), for the sparse index the MLM head's largest terms of each.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "abi.h"
#include "host_chunks.h"

namespace bert_hip {

// Tokenizes and evaluates texts in groups on the context's first device; each group's embeddings [c][n_embd] land in the
// index's device scratch buffer and are handed to use(i0, c, d_rows).  No host copy of the embeddings.
template <class F>
bool encode_groups_device(bert_ctx *ctx, Index &ix, int32_t n_threads, int32_t n, const char **texts, F &&use, std::string &err) {
    const int32_t H = ctx->hp.n_embd, G = 16384;
    TokenGroup &g = ctx->texts.group[0];
    for (int32_t i0 = 0; i0 < n; i0 += G) {
        const int32_t c = std::min(G, n - i0);
        g.tokenize(ctx->texts, n_threads, c, texts + i0);
        if (g.n_ok < c) { err = "input " + std::to_string(i0 + g.n_ok) + " cannot be evaluated"; return false; }
        float *d = ix.scratch((size_t)c * H, err);
        if (!d) return false;
        // (blocking: the rows are in d when it returns)
        if (ctx->engine()->eval_packed_host(g.packed.get(), g.cu.data(), c, nullptr, err, d) != 0) return false;
        if (!use(i0, c, d)) return false;
    }
    return true;
}

// the multi-device route of the text entry points: bert_hip_encode_batch into host rows
inline bool encode_host(bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, std::vector<float> &emb, std::string &err) {
    const size_t H = ctx->hp.n_embd;
    emb.assign((size_t)n * H, 0.f);
    std::vector<float *> rows((size_t)n);
    for (int32_t i = 0; i < n; ++i) rows[i] = emb.data() + i * H;
    const int32_t done = encode_batch_impl(ctx, n_threads, n, texts, rows.data());
    if (done != n) { err = "input " + std::to_string(std::max(done, 0)) + " could not be encoded"; return false; }
    return true;
}

// what the sparse text routes ask of the model (false + err otherwise)
inline bool text_model_ok(const bert_ctx *ctx, const SparseIndex &x, std::string &err) {
    if (!ctx->engine()->has_mlm_head()) { err = "the model file has no MLM head (cls.predictions.*)"; return false; }
    if (x.n_vocab() != ctx->hp.n_vocab) { err = "the index has n_vocab " + std::to_string(x.n_vocab()) + ", the model's is " + std::to_string(ctx->hp.n_vocab); return false; }
    return true;
}

// The way from texts to chunks in an index's device buffers, for the sparse index (below) and the token index (token_index_api.cpp).
// Tokenizes the texts in groups of 4096, hands every group to pre(i0, m, cu) — nonzero: returned at once —, cuts it by the chunk rule
// (host_chunks.h; max_sentences: its cap, 0 for none), and per chunk of nb sentences and T tokens: the staging block (ids | cu_seqlens)
// into the index's device buffer by one copy, out_bytes(nb, T) bytes of room in its other one, then
// use(i0, nb, T, max_len, h_cu, d_ids, d_cu, d_out) — i0: the chunk's first text; h_cu: the chunk's cu_seqlens from 0, host; d_ids / d_cu:
// the same on the device — all on the index's stream, which is synchronised behind every chunk.  0, or what pre or use returned, or
// -2 / -3 (+ err).
template <class Ix, class Pre, class OutBytes, class F>
int32_t text_chunks(bert_ctx *ctx, Ix &x, int32_t n_threads, int32_t n, const char **texts, int max_sentences, Pre &&pre, OutBytes &&out_bytes, F &&use,
                    std::string &err) {
    constexpr int32_t GROUP = 4096;
    TokenGroup &g = ctx->texts.group[0];
    std::vector<char> block;
    for (int32_t i0 = 0; i0 < n; i0 += GROUP) {
        const int32_t m = std::min(GROUP, n - i0);
        g.tokenize(ctx->texts, n_threads, m, texts + i0);
        if (g.n_ok < m) { err = "input " + std::to_string(i0 + g.n_ok) + " cannot be evaluated"; return -2; }
        const int32_t *cu = g.cu.data();
        if (const int32_t r = pre(i0, m, cu)) return r;
        for (int b0 = 0; b0 < m;) {
            const HostChunk c = next_host_chunk(cu, m, b0, ctx->engine()->options().chunk_tokens, max_sentences);
            const int nb = c.b1 - b0, T = cu[c.b1] - cu[b0];
            const StagingLayout L(T, nb, false, 0);
            char *d_in = nullptr, *d_out = nullptr;
            if (!x.text_buffers(L.bytes, out_bytes(nb, T), d_in, d_out, err)) return -3;
            block.resize(std::max(block.size(), L.bytes));
            const int32_t *h_cu = fill_staging(block.data(), L, g.packed.get(), cu, c, nullptr, nullptr, 0);
            hipStream_t s = x.stream();
            // (a pageable source: the copy has left the block when it returns)
            if (hipMemcpyAsync(d_in, block.data(), L.bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
                (void)hipStreamSynchronize(s);
                err = "hipMemcpyAsync (ids) failed";
                return -3;
            }
            int32_t r = use(i0 + b0, nb, T, c.max_len, h_cu, (const int32_t *)d_in, (const int32_t *)(d_in + L.off_cu), d_out);
            if (hipStreamSynchronize(s) != hipSuccess && r == 0) { err = "device error"; r = -3; }
            if (r != 0) return r;
            b0 = c.b1;
        }
    }
    return 0;
}

// The sparse text route: chunks capped at the sentences whose terms fit 32 MiB; per chunk the MLM head's k largest terms of every text
// into the index's output buffer (ids [nb][k] | weights [nb][k]), then use(i0, nb, d_ids, d_weights).  0, -2 or -3 (+ err).
template <class F>
int32_t sparse_text_chunks(bert_ctx *ctx, SparseIndex &x, int32_t n_threads, int32_t n, const char **texts, int32_t k, F &&use, std::string &err) {
    auto off_w = [k](int nb) { return ((size_t)nb * k * 4 + 15) & ~(size_t)15; };
    return text_chunks(ctx, x, n_threads, n, texts, std::max(1, (int)(((size_t)32 << 20) / ((size_t)k * 8))),
        [](int32_t, int32_t, const int32_t *) { return 0; }, [&](int nb, int) { return off_w(nb) + (size_t)nb * k * 4; },
        [&](int32_t i0, int nb, int T, int max_len, const int32_t *, const int32_t *d_ids, const int32_t *d_cu, char *d_out) -> int32_t {
            if (ctx->engine()->sparse_packed_device(d_ids, d_cu, nb, T, max_len, k, (int32_t *)d_out, (float *)(d_out + off_w(nb)), x.stream(), err) != 0) return -3;
            return use(i0, nb, (const int32_t *)d_out, (const float *)(d_out + off_w(nb)));
        }, err);
}

}  // namespace bert_hip
