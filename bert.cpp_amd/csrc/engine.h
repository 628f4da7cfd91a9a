// engine.h — device side of a bert_ctx: HBM-resident weights, workspace, and the launch sequence
// of the forward pass.  Replaces the reference's ggml arena + per-sentence graph build + execute
// (reference bert.cpp:730-941, sizing :680-713) with a fixed kernel sequence over a packed variable-length batch: by default
// one launch for all layers behind the embedding kernel, else two fused launches per layer (plan() in engine.hip picks the route).
// The weights are weights.h's, the switches options.h's, the per-kernel times profiler.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"
#include "model_file.h"
#include "options.h"
#include "profiler.h"
#include "weights.h"

namespace bert_hip {

class Engine {
public:
    // device: HIP ordinal the weights are uploaded to and every launch runs on
    static Engine *create(const ModelFile &mf, int device, std::string &err);
    ~Engine();

    // host-resident packed batch (validated by the caller), blocking
    // embeddings: host destination [n_sentences][H]; d_embeddings (optional, instead): destination in this device's memory
    // pool_mode: as for eval_packed_device below
    int eval_packed_host(const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, float *embeddings,
                         std::string &err, float *d_embeddings = nullptr, int pool_mode = -1);
    // device-resident, asynchronous on `stream`
    // d_windows / n_windows: optional sentence windows of the fused projection+attention kernel (build_windows), in
    // device memory; without them the same windows are built on the device (launch_build_windows) when the batch is
    // short enough on average for packing to pay, else sentences are placed by the uniform rule of qkv_attention2.hip
    int eval_packed_device(const int32_t *d_tokens, const int32_t *d_cu, int n_sentences, int n_tokens, int max_len,
                           float *d_out, hipStream_t stream, float *d_hidden, std::string &err,
                           const int2 *d_windows = nullptr, int n_windows = 0, int window_slots = 0,       // window_slots: the place granularity d_windows was built with (0: read it now)
                           int pool_mode = -1,                   // kernels.h POOL_*: what the host call read for all its chunks (-1: read the options now)
                           void *d_token_rows = nullptr, int token_flags = 0,      // token rows (below); d_out may then be null: the embeddings stay in d_out_
                           const int32_t *d_first_len = nullptr);                  // token types (below); null: type 0 everywhere, the untyped embedding kernels
    // Sentence pairs and scores (bert_hip.h): a TYPED pass carries d_first_len [n_sentences] — the leading tokens of each sentence that take
    // token-type row 0, the rest row 1 (kernels.h launch_embed_ln) — and plans like any other pass; only the embedding launch differs.
    // score_packed_device: a typed pass that ends in POOL_CLS | POOL_RAW rows in d_out_ (the mode handed in as an argument, as the grouped
    // pass hands in POOL_RAW; the options stay as they are), then the head launch ("cls_head" in the profile; cls_head.hip: the
    // matrix-core form, or the plain form on the f32 route and for an H the other refuses) -> d_scores f32 [n_sentences][n_labels].
    // flags: kernels.h CLS_HEAD_SIGMOID.  -2 with a message for a model without a head.  After reserve() it allocates nothing.
    int n_labels() const { return w_->n_labels; }
    int score_packed_device(const int32_t *d_tokens, const int32_t *d_cu, const int32_t *d_first_len, int n_sentences, int n_tokens, int max_len,
                            int flags, float *d_scores, hipStream_t stream, std::string &err,
                            const int2 *d_windows = nullptr, int n_windows = 0, int window_slots = 0);      // (as eval_packed_device takes them)
    // Host forms, blocking, on this engine's device: cut at chunk_tokens between sentences, one copy per chunk and direction (ids |
    // cu_seqlens | first_len in; rows or scores out).  first_len: nullable (all type 0), validated by the caller.  scores == false: the
    // context's pooling and normalisation, out [n_sentences][H]; true: out [n_sentences][n_labels].
    int eval_packed_typed_host(const int32_t *tokens, const int32_t *cu_seqlens, const int32_t *first_len, int n_sentences, bool scores, int flags,
                               float *out, std::string &err);
    // Learned sparse embeddings (bert_hip.h): a pass planned as a token-rows pass — its final states stay in x_ in row order, nothing is
    // copied (eval_packed_device is handed x_ itself as the rows' destination) —, then the MLM transform t = LayerNorm(gelu(x Wt^T + bt))
    // into ctx_, free behind the pass ("mlm_transform", "mlm_layernorm" in the profile: launch_gemm_mfma / _naive + launch_layernorm, or
    // the f32 route's two), then the vocabulary launch on the tied word embeddings (sparse_vocab.hip: "sparse_vocab" + "sparse_finish";
    // the plain form on the f32 route and for an H the other refuses).  k == 0: d_weights f32 [n_sentences][n_vocab], d_ids unused.
    // 1 <= k <= SPARSE_MAX_K: the head runs in chunks of sparse_chunk() sentences into sparse_dense_ and "sparse_topk" selects from
    // each: d_ids i32 [n_sentences][k], d_weights f32 [n_sentences][k].  -2 with a message for a model without the head.  After
    // reserve() it allocates nothing: reserve fixes the chunk and sizes sparse_dense_ with the workspace.
    bool has_mlm_head() const { return w_->mlm_head; }
    bool has_rel_bias() const { return w_->rel_bias; }
    int sparse_packed_device(const int32_t *d_tokens, const int32_t *d_cu, int n_sentences, int n_tokens, int max_len, int k, int32_t *d_ids,
                             float *d_weights, hipStream_t stream, std::string &err);
    // Host form, blocking, on this engine's device: cut at chunk_tokens between sentences and at the sentences whose results fit 32 MiB,
    // one plain copy per chunk and direction.  k == 0: weights [n_sentences][n_vocab], ids unused.
    int sparse_packed_host(const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, int k, int32_t *ids, float *weights, std::string &err);
    // Token rows (bert_hip.h "token rows and late interaction"): a pass with one more destination, [n_tokens][H] rows of the final states
    // (kernels.h launch_token_rows, TOKEN_ROWS_* flags), written by one launch ("token_rows" in the profile) beside the pooling launch.
    // Such a pass does not take the one-launch kernel (which keeps x on chip between its phases and pools inside the launch: the other
    // routes leave the final states in x_ in row order); LayerNorm folding stays as planned, so the embeddings are eval_packed's bits.
    // Host form, blocking, on this engine's device: cut at chunk_tokens between sentences, one plain copy per chunk and direction.
    // flags: TOKEN_ROWS_NORMALIZE only (rows are f32).  embeddings: nullable.
    int eval_packed_tokens_host(const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, int flags, float *rows, float *embeddings,
                                std::string &err);
    // next-fit packing of whole sentences (in order, each starting at a multiple of 16 slots) into windows of 128 token
    // slots: {first sentence, count} per window.  Sentences longer than a window get one of their own (the fused kernel is
    // not used for such batches).
    static void build_windows(const int32_t *cu_seqlens, int n_sentences, std::vector<int2> &windows, int slots);
    int eval_hidden(const int32_t *tokens, int n_tokens, float *hidden, float *embedding, std::string &err);

    // Grouped pooling (bert_hip.h "long texts"): the pass runs with POOL_RAW handed in as an argument (the options stay as they
    // are), its rows go to raw_rows_ and launch_group_pool makes one row of every group of consecutive sentences, by the context's
    // "pooling" (token-count or unit weights) and "normalize", both read once per call.  group_cu: n_groups + 1 entries.
    // Host form, blocking: group_cu validated by the caller; embeddings: host destination [n_groups][H], or d_embeddings: one in this
    // device's memory.  h_raw_rows (optional): the sentences' POOL_RAW rows [n_sentences][H] in host memory, computed elsewhere (a
    // multi-device context's sharded pass) under pool_mode: no pass here, they are uploaded and pooled.
    int eval_packed_grouped_host(const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, const int32_t *group_cu, int n_groups,
                                 float *embeddings, float *d_embeddings, std::string &err, const float *h_raw_rows = nullptr, int pool_mode = -1);
    // Device form, asynchronous on `stream`.  raw_rows_ grows on demand like the workspace (eval_packed_device)
    int eval_packed_grouped_device(const int32_t *d_tokens, const int32_t *d_cu, int n_sentences, int n_tokens, int max_len,
                                   const int32_t *d_group_cu, int n_groups, float *d_out, hipStream_t stream, std::string &err);

    // sizes the workspace for batches of up to n_tokens tokens / n_sentences sentences now, so that later calls of
    // eval_packed_device never allocate (allocation synchronises the device and breaks stream capture)
    bool reserve(int n_tokens, int n_sentences, std::string &err);
    // device-side validation (sentence lengths vs max_len): synchronises, returns and clears the status word
    int check(std::string &err);
    void set_option(const std::string &key, const std::string &value);
    void profile_enable(bool on) { prof_.enable(on); }
    std::string profile_report();
    // a launch of another part of the library (the index kernels of search.hip) under this engine's profiling: listed by
    // profile_report as `name`
    void timed_launch(const char *name, double flops, hipStream_t s, const std::function<void()> &f);

    // The one-event rule and stream capture (bert_hip.h "stream capture and graphs"), in one place for the engine and its indexes.  An
    // operation that uses this engine's workspace, or the buffers of one of its indexes, starts with op_begin on the caller's stream and
    // ends with op_end; `busy` is the owner's event (null: the operation shares no buffer, as MaxSim).
    //   eager:      op_begin makes s wait for busy, op_end records busy on s — operations never overlap, whatever their streams
    //   capturing:  neither touches busy.  A wait inside a capture for an event recorded on the same stream before it fails
    //               (hipErrorStreamCaptureIsolation) and invalidates the capture; an event recorded inside a capture belongs to the
    //               capture, which the blocking paths' hipEventSynchronize (grow, compact, save, the destructor) need not accept; and
    //               a replay records nothing anyway.  Inside one capture the stream orders the operations; against everything else
    //               the caller orders the graph launch.
    //   capturing while the engine profiles: refused (false, a message in err, nothing enqueued) — a timed launch carries an
    //               event pair that a capture would take over in the same way, and hipEventElapsedTime on them is undefined.
    struct StreamOp { hipStream_t s = nullptr; hipEvent_t busy = nullptr; bool capturing = false; };
    bool op_begin(hipStream_t s, hipEvent_t busy, StreamOp &op, std::string &err);
    bool op_end(const StreamOp &op, std::string &err);

    const HParams &hparams() const { return hp_; }
    const EngineOptions &options() const { return opt_; }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }

private:
    Engine() = default;
    bool ensure_workspace(int t_pad, int n_sentences, std::string &err);
    // sentences whose dense rows [n_vocab] f32 fit 32 MiB, at least one: what bounds sparse_dense_ and a host chunk's results
    int sparse_sentence_cap() const { return std::max(1, (int)(((size_t)32 << 20) / ((size_t)hp_.n_vocab * 4))); }
    bool ensure_sparse(int n_sentences, std::string &err);    // grows sparse_chunk_ (never past the cap) and sparse_dense_ with it

    // The forward pass: plan() decides everything once, before the first launch; a forward_* method per route only launches.
    enum class Route { F32, LATENCY, ONE_LAUNCH, FOLDED, LAYERED };
    enum class Family { GEMM256, MFMA, NAIVE, F32 };         // the kernel that serves a weight mat-mul
    struct LayerPlan {                                       // (LAYERED; FOLDED reads layer 0's planes)
        bool qkv2 = false;            // qkv_attention2, else the Q|K|V mat-mul + attention
        bool tail = false;            // layer_tail, else the mat-muls + LayerNorms
        bool planes = false;          // the Q|K|V mat-mul reads the 4-bit planes (LayerWeights::qkv_q4), else the f16 image
        Family qkv = Family::NAIVE, o = Family::NAIVE, ffi = Family::NAIVE, ffo = Family::NAIVE;
    };
    struct Plan {
        // the call (windows, n_windows: the caller's list, or the one the pass builds on the device)
        const int32_t *tokens, *cu;
        int B, T, max_len, t_pad, slots, pool_mode;
        float *out, *hidden;
        void *token_rows;             // token rows wanted (eval_packed_device): no one-launch kernel
        const int32_t *first_len;     // a typed pass (eval_packed_device): the embedding launch's first_len, else null
        hipStream_t s;
        const int2 *windows;
        int n_windows;
        // the decisions
        Route route = Route::LAYERED;
        bool build_windows = false;   // launch_build_windows ahead of the route, its count in n_windows_dev (n_windows: a bound)
        const int *n_windows_dev = nullptr;
        bool embed_lanes = false;     // ONE_LAUNCH on full windows: the embedding kernel writes y_ in lane order, x_ is not written (model_kernel.hip)
        std::vector<LayerPlan> layers;
    };
    Plan plan(const int32_t *d_tokens, const int32_t *d_cu, int B, int T, int max_len, float *d_out, hipStream_t s, float *d_hidden,
              const int2 *d_windows, int n_windows, int slots, int pool_mode, void *d_token_rows = nullptr, const int32_t *d_first_len = nullptr) const;
    bool forward_f32(const Plan &p, std::string &err);        // f32 files in f32 arithmetic (f32_route.hip), one launch per operation
    void forward_latency(const Plan &p);
    void forward_one_launch(const Plan &p);
    bool forward_folded(const Plan &p, std::string &err);
    bool forward_layers(const Plan &p, std::string &err);
    // A, resid, C: f32 for Family::F32, else f16
    bool gemm(const Plan &p, const char *name, Family f, const GemmWeightStore &W, const void *A, const float *bias, const void *resid, void *C,
              int epi, std::string &err, const GemmLnFold *ln = nullptr);
    void attention(const Plan &p);
    void tap(const Plan &p, int idx);
    // the grouped-pooling launch ("group_pool" in the profile) behind a pass on s, then busy_ again: the next pass must not write raw_rows_ under it
    int group_pool(const int32_t *d_cu, int n_sentences, const int32_t *d_group_cu, int n_groups, float *d_out, int pool_mode, const StreamOp &op, std::string &err);
    template <class F> void timed(const char *name, double flops, hipStream_t s, F &&f) { prof_.timed(name, flops, s, f); }

    HParams hp_;
    int device_ = 0;
    EngineOptions opt_;
    std::unique_ptr<ModelWeights> w_;
    LaunchProfiler prof_;

    // workspace (grow-only)
    DevBuf x_, qkv_, ctx_, y_, ff_, v32_, d_tokens_, d_cu_, d_out_, d_hidden_, status_, windows_;
    DevBuf typed_in_, typed_out_;                             // the host forms of the typed pass: a chunk's ids | cu_seqlens | first_len, and its rows or scores
    DevBuf sparse_dense_, sparse_in_, sparse_out_;           // learned sparse embeddings: the top-k form's dense rows [sparse_chunk_][n_vocab] f32; the host form's ids | cu_seqlens and its results
    int sparse_chunk_ = 0;
    DevBuf tok_in_, tok_rows_;                                // the host form of the token rows: a chunk's ids | cu_seqlens, and its rows
    DevBuf raw_rows_, group_in_, group_out_;                  // grouped pooling: the sentences' POOL_RAW rows [n_sentences][H] f32; the host form's cu_seqlens | group_cu and its groups' rows
    DevBuf ln_stats1_, ln_stats2_, ln_rows1_, ln_rows2_;      // LayerNorm folding: per-row partial statistics / finalized rows of the two LayerNorms of a layer
    hipStream_t stream_ = nullptr;
    // the workspace serves ONE forward pass at a time: every pass waits for the previous one's event on its own stream
    hipEvent_t busy_ = nullptr;
    // host path: two sets of pinned staging + device id / embedding buffers, so that the host stages chunk i+1 and
    // unpacks chunk i-1 while the GPU computes chunk i (eval_packed_host)
    struct HostSlot {
        // ONE pinned staging block per chunk — ids | cu_seqlens | windows, each part 16-byte aligned — and one device image of
        // it: a single H2D copy per chunk.  The embeddings come back without a copy: the pooling kernel writes them straight
        // into h_out (pinned, mapped into the device's address space as d_out_host).
        char *h_in = nullptr, *d_in_host = nullptr;          // (d_in_host: h_in as the device sees it)
        float *h_out = nullptr, *d_out_host = nullptr;
        size_t h_in_cap = 0, h_out_cap = 0;
        DevBuf d_in, d_out;
        hipEvent_t done = nullptr;
    } slot_[2];
};

}  // namespace bert_hip
