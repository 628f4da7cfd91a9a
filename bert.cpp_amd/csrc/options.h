// options.h — the switches of an engine, and their two spellings: the BERT_HIP_* environment (read once, when a model loads)
// and the keys of bert_hip_set_option.  INTEGRATION.md lists both for users.
#pragma once
#include <initializer_list>
#include <string>

#include "model_file.h"

namespace bert_hip {

struct DevBuf;

struct EngineOptions {
    bool gemm_naive = false, attn_naive = false;      // the generic kernels (libbert_test.so only)
    bool qkv2 = true, gemm256 = true, tail = true;
    bool ln_fold = true;              // H = 768 route: LayerNorm folded into the mat-muls (needs the images: built at load)
    bool latency = true;
    bool q4_expand = true;            // q4 files: f16 images and f32 tables built at load (no key: load time only)
    bool f32_exact = true;            // f32 files take the f32 route unless BERT_HIP_F32=f16 / "f32" = "f16"
    int one_launch = 1;               // all layers in one launch: 0 never, 1 when it pays (well-filled windows), 2 whenever the kernel takes the batch
    int chunk_tokens = 262144;
    // Calls of at most this many tokens take the latency route (skinny.hip).  A call of T tokens keeps ceil(T / 128) CUs busy on
    // the fused kernels — 615-685 us for anything from 129 to 3000 tokens of all-MiniLM-L6-v2 — while the route's time grows with T
    // from 220 us: 252 us at 172 tokens (8 sentences), 330 at 363 (16), 376 at 512, 527 at 716, 606 at 1024 (round 5, same bits).
    int latency_tokens = 768;
    int sparse_index_qb = 0;          // tuning (a key only): queries per tile of the sparse index's scan, 1 .. 8; 0 = the table of sparse_index_kernels.h
    int sparse_index_segment_rows = 0; // tuning (a key only): rows per segment of the sparse index's postings, 256 .. 16384 in multiples of 256, read by invert; 0 = the default of sparse_index_kernels.h
    int hybrid_chunk_queries = 0;     // tuning (a key only): queries per chunk of a hybrid search, 1 .. 4096; 0 = what the score workspace's bound gives (sparse_index_kernels.h)
    int token_index_slices = 0;       // tuning (a key only): slices of documents of a token index's scan, 1 .. 4096; 0 = planned (token_index_kernels.h)
    int maxsim_launch_pairs = 0;      // tuning (a key only): pairs per launch of MaxSim's kernel, 1 .. 2^23 (a larger value is clamped to that bound); 0 = the bound (kernels.h)
    bool stage_kernel = true;       // small staged blocks come in by a kernel that reads the mapped pinned block, not by the copy engine
    // How a pass ends (bert_hip.h): the mean over a sentence's tokens or the state of its first token ([CLS]), divided by its L2
    // norm or not.  A pass reads both once, at its start (pool_mode()).
    bool pool_cls = false, normalize = true;
    int pool_mode() const;            // kernels.h: POOL_CLS | POOL_RAW

    // the defaults for a model of these dimensions, then the environment
    static EngineOptions from_env(const HParams &hp);
    // a key of bert_hip_set_option.  naive_images / fold_images: what was built at load (ModelWeights) — "gemm" = "naive" and
    // "ln_fold" = "1" are refused, with a line on stderr, without them.  Unknown keys are ignored; so is, with a line on stderr, a value
    // that "pooling" or "normalize" do not know (from the environment as well).
    void set(const std::string &key, const std::string &value, bool naive_images, bool fold_images);

private:
    void apply(const std::string &key, const std::string &value);
};

// "test_poison_ctx" (libbert_test.so only; false, doing nothing, in libbert.so): every half of the attention-context workspace
// becomes a NaN, so a pass that still reads what it has not written itself shows it in its results.  "test_poison_xres": the same for the
// workspace the one-launch kernel's full form starts from and passes the residual between its layers through (the engine's y rows: the
// pass's embedding kernel writes them first, in lane order).
// "test_poison_workspace": the same for every activation scratch buffer of the engine at once (`workspace`: x, qkv, ctx, y, the
// intermediate, the latency route's f32 rows, the LayerNorm fold's partial statistics and finalized rows, the hidden-state tap's
// rows; f32 words on the f32 route, where 0xFF bytes are a NaN as well) — a pass may depend on nothing it finds in any of them:
// not on the rows behind its last token, not on rows a kernel of its own has yet to write.  Left out: the buffers a pass does not
// compute (token ids, cu_seqlens, the staged input blocks, the window list, the embeddings and the status words).  The engine has no
// buffer that it fills once and then relies on across passes (DevBuf::ensure zero-fills what it allocates, and no kernel may count on
// those zeros: the first pass that reaches a row overwrites them), so nothing else is exempt.
bool test_poison_option(const std::string &key, const DevBuf &ctx, const DevBuf &xres, std::initializer_list<const DevBuf *> workspace);

}  // namespace bert_hip
