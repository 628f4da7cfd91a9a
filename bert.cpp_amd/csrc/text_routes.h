// text_routes.h — how the text entry points of the two indexes (index_api.cpp, sparse_index_api.cpp) and of the hybrid search
// (hybrid_api.cpp) get from texts to device buffers: the embeddings of a group of texts into the embedding index's scratch buffer,
// the MLM head's largest terms of a chunk of texts into the sparse index's text buffers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "abi.h"

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

// Tokenizes the texts in groups of 4096, cuts each group at chunk_tokens between sentences and at the sentences whose terms fit
// 32 MiB, and per chunk: ids | cu_seqlens into the index's device buffer, the MLM head's k largest terms of every text into its other
// one (ids [nb][k] | weights [nb][k]), then use(i0, nb, d_ids, d_weights) — all on the index's stream.  0, -2 or -3 (+ err).
template <class F>
int32_t sparse_text_chunks(bert_ctx *ctx, SparseIndex &x, int32_t n_threads, int32_t n, const char **texts, int32_t k, F &&use, std::string &err) {
    constexpr int32_t GROUP = 4096;
    Engine *eng = ctx->engine();
    TokenGroup &g = ctx->texts.group[0];
    const int cap = std::max(1, (int)(((size_t)32 << 20) / ((size_t)k * 8)));
    std::vector<int32_t> h_cu;
    for (int32_t i0 = 0; i0 < n; i0 += GROUP) {
        const int32_t m = std::min(GROUP, n - i0);
        g.tokenize(ctx->texts, n_threads, m, texts + i0);
        if (g.n_ok < m) { err = "input " + std::to_string(i0 + g.n_ok) + " cannot be evaluated"; return -2; }
        const int32_t *cu = g.cu.data();
        for (int b0 = 0; b0 < m;) {
            int b1 = b0 + 1, max_len = cu[b0 + 1] - cu[b0];
            while (b1 < m && b1 - b0 < cap && cu[b1 + 1] - cu[b0] <= eng->options().chunk_tokens) { max_len = std::max(max_len, cu[b1 + 1] - cu[b1]); ++b1; }
            const int nb = b1 - b0, T = cu[b1] - cu[b0];
            const size_t off_cu = ((size_t)T * 4 + 15) & ~(size_t)15, off_w = ((size_t)nb * k * 4 + 15) & ~(size_t)15;
            char *d_in = nullptr, *d_out = nullptr;
            if (!x.text_buffers(off_cu + (size_t)(nb + 1) * 4, off_w + (size_t)nb * k * 4, d_in, d_out, err)) return -3;
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
            int32_t r = eng->sparse_packed_device((const int32_t *)d_in, (const int32_t *)(d_in + off_cu), nb, T, max_len, k, (int32_t *)d_out,
                                                  (float *)(d_out + off_w), s, err) != 0 ? -3 : 0;
            if (r == 0) r = use(i0 + b0, nb, (const int32_t *)d_out, (const float *)(d_out + off_w));
            if (hipStreamSynchronize(s) != hipSuccess && r == 0) { err = "device error"; r = -3; }
            if (r != 0) return r;
            b0 = b1;
        }
    }
    return 0;
}

}  // namespace bert_hip
