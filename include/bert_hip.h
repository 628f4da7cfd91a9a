/* bert_hip.h — extensions of the MI355X engine beyond the reference's bert.h.
 *
 * Plain C ABI (pointers + sizes, no torch / HIP types in the signatures; a stream is passed as a
 * `void *` that must be a hipStream_t or NULL for the default stream).  None of these exist in
 * skeskinen/bert.cpp; each entry names the reference code it generalises.
 */
#ifndef BERT_HIP_H
#define BERT_HIP_H

#include "bert.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tokenizer-only context: header + vocab of a model file, no weights, no GPU needed.
 * bert_tokenize / bert_vocab_id_to_token / bert_n_max_tokens work; eval prints an error.
 * (Tokenization is CPU-only in the reference as well: bert.cpp:199-325.)                        */
BERT_API struct bert_ctx *bert_hip_load_tokenizer(const char *fname);

/* bert_tokenize for many texts on up to n_threads host threads (what bert_encode_batch does before it evaluates):
 * tokens[i * bert_n_max_tokens(ctx) ..] receives the ids of texts[i], n_tokens[i] their count.  Works on
 * tokenizer-only contexts.  Returns 0, negative on bad arguments.                                             */
BERT_API int32_t bert_hip_tokenize_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts,
                                         bert_vocab_id *tokens, int32_t *n_tokens);

/* Model facts from the file header (reference bert.cpp:361-367).                                */
BERT_API int32_t bert_hip_n_layer(struct bert_ctx *ctx);
BERT_API int32_t bert_hip_n_head(struct bert_ctx *ctx);
BERT_API int32_t bert_hip_n_intermediate(struct bert_ctx *ctx);
BERT_API int32_t bert_hip_n_vocab(struct bert_ctx *ctx);
BERT_API int32_t bert_hip_ftype(struct bert_ctx *ctx);        /* 0 f32, 1 f16, 2 q4_0, 3 q4_1 */
BERT_API int32_t bert_hip_device(struct bert_ctx *ctx);       /* HIP ordinal of the context's first device, -1 if none */
BERT_API int32_t bert_hip_n_devices(struct bert_ctx *ctx);    /* GPUs the context spreads its batches over */
/* How the context's passes end ("pooling" / "normalize" below); -1 for a context without a device (tokenizer-only, NULL).       */
BERT_API int32_t bert_hip_pooling(struct bert_ctx *ctx);      /* 0 mean, 1 cls */
BERT_API int32_t bert_hip_normalize(struct bert_ctx *ctx);    /* 1 the embedding is divided by its L2 norm, 0 it is not */

/* bert_encode_batch with a result: the number of inputs encoded (all of them, or the inputs in front of the first one
 * that could not be evaluated — later embeddings stay untouched), negative on an internal error.                     */
BERT_API int32_t bert_hip_encode_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts,
                                       float **embeddings);

/* Packed, variable-length batch evaluation — the engine's native entry point; bert_eval_batch
 * (reference bert.cpp:730-941) is a wrapper that packs the per-sentence host pointers.
 *   tokens      [n_tokens_total] ids of all sentences back to back
 *   cu_seqlens  [n_sentences + 1] exclusive prefix sums of the sentence lengths (cu[0] = 0)
 *   embeddings  [n_sentences * bert_n_embd] row-major
 * Returns 0 on success, negative on error (message on stderr, outputs untouched).               */
BERT_API int32_t bert_hip_eval_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens,
                                      const int32_t *cu_seqlens, int32_t n_sentences, float *embeddings);

/* Multi-GPU contexts (BERT_HIP_DEVICES=all or a list; default: the calling thread's current device only): bert_eval_batch / bert_encode_batch /
 * bert_hip_eval_packed cut a call into contiguous shards with near-equal token counts, one per device (weights are
 * replicated, each device has its own host thread and stream), and every shard writes its embeddings straight into
 * the caller's host rows.  bert_hip_eval_packed_gather keeps the results on the devices instead and runs the path's one
 * exchange step — an RCCL all-gather over xGMI (librccl.so is loaded, and the communicator made, when the model is loaded) — so that afterwards EVERY device
 * holds the whole [n_sentences][n_embd] f32 matrix: d_embeddings[d] receives the pointer on device d (owned by the
 * context, valid until the next call; bert_hip_n_devices entries).  Blocking.  Per-sentence results are the same bits
 * whatever the number of devices.  Returns 0, negative on error.                                                      */
BERT_API int32_t bert_hip_eval_packed_gather(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens,
                                             int32_t n_sentences, float **d_embeddings);

/* Same computation with every buffer already resident in HBM on the context's FIRST device; work is
 * enqueued on `stream` and NOT synchronised (the caller owns the stream).  `max_len` must be >=
 * the longest sentence (it selects and sizes the attention kernels); n_tokens_total = cu[n].
 * Rules of the asynchronous entry point:
 *   - a context has ONE workspace: an eagerly enqueued forward pass waits (on its own stream, hipStreamWaitEvent) for the
 *     previous eagerly enqueued pass of the context, whatever stream that ran on — eager passes never overlap and need no
 *     extra ordering.  A pass that runs as part of a graph launch is outside this rule: the caller orders it (STREAM CAPTURE
 *     AND GRAPHS below);
 *   - the workspace grows on demand, and growing allocates (synchronises the device, illegal under stream capture):
 *     call bert_hip_reserve once with the largest batch first;
 *   - lengths are validated on the device: a sentence longer than max_len (or empty) yields a NaN embedding and sets a
 *     status word that bert_hip_check returns (and clears) after synchronising.  A batch shaped like full windows
 *     (n_tokens_total = 128 n_sentences, max_len = 128) is evaluated 128-token block by block: if it has that shape only by
 *     the sum of its lengths (an over-long sentence, a shorter one), every sentence that is not exactly its block gets a
 *     NaN row as well — the other rows are the bits they always have;
 *   - short sentences are packed several to a 128-slot attention window by a kernel of the pass itself (the lengths
 *     exist only in HBM here): results are the bits of the host entry points.                                        */
BERT_API int32_t bert_hip_eval_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens,
                                             const int32_t *d_cu_seqlens, int32_t n_sentences,
                                             int32_t n_tokens_total, int32_t max_len,
                                             float *d_embeddings, void *stream);

BERT_API int32_t bert_hip_reserve(struct bert_ctx *ctx, int32_t n_tokens, int32_t n_sentences);
BERT_API int32_t bert_hip_check(struct bert_ctx *ctx);        /* 0 ok, 1 a batch broke its max_len promise, < 0 error */

/* STREAM CAPTURE AND GRAPHS.  Every *_device entry point of this header may be called on a stream that is capturing (hipStreamBeginCapture;
 * a capture on ONE stream), provided the call does not have to allocate: size the context with bert_hip_reserve and an index with
 * bert_hip_index_reserve, and call once eagerly at the largest shape where an entry says that those two do not cover its buffer (grouped
 * pooling, rescore, the probed and the two-stage searches).  The captured call returns 0 and runs nothing; the graph holds its launches,
 * all of them on the caller's stream.
 *   A graph bakes in what the host knew at capture: n_sentences, n_tokens_total and max_len; the route and every option the pass read
 *   ("pooling", "normalize", the kernel switches, "window_slots"); n_queries, k, nprobe, n_cand and n_words; the index's row count, its
 *   partition and its storage pointers; the workspace pointers of the context and of the index.  None of these can change between
 *   replays.  So whatever grows, moves or frees that memory invalidates the graph, and launching it afterwards reads freed memory:
 *   bert_hip_reserve or an eager call beyond the reserved size, bert_hip_index_reserve, an add beyond the capacity, compact, partition,
 *   bert_hip_index_free, bert_free.  An add within the capacity keeps the graph valid, but the graph goes on searching the rows it was
 *   captured with.
 *   What may change between replays is the CONTENTS of the caller's device buffers: ids, cu_seqlens and group_cu (the lengths are read on
 *   the device: any lengths with the same n_sentences and the same sum; the max_len guard and bert_hip_check work as in an eager call),
 *   queries, allow-list bits, candidate ids, token rows, pairs.  A replay gives the bits of the eager call on the same buffers.
 *   bert_hip_index_add_device under capture returns the first id and grows size WHEN IT IS CAPTURED, not when the graph runs; every launch
 *   converts what d_rows holds then into those same rows (a second launch overwrites them, it does not append).  A search captured behind
 *   it in the same capture sees them; before the first launch those rows are undefined.
 *   Ordering.  The one-event rule (one pass of a context, one operation of an index at a time, whatever the streams) orders EAGER calls
 *   only: a captured call neither waits for the event nor records it — an event recorded inside a capture belongs to that capture, and a
 *   replay would record nothing anyway.  Inside one capture the stream orders the operations.  The caller orders every graph launch against
 *   every other use of the same context or index: eager calls on other streams, the host entry points (which run on streams of the
 *   context's own), other graphs.
 *   Profiling and capture exclude each other: while bert_hip_profile_enable is on, a *_device call on a capturing stream returns -3 after
 *   one line on stderr and enqueues nothing; the capture stays valid.
 *   A call that has to allocate under capture fails with -3 (hipMalloc: hipErrorStreamCaptureUnsupported) and the runtime invalidates the
 *   capture: hipStreamEndCapture returns hipErrorStreamCaptureInvalidated and no graph.  The context and its indexes are unharmed — reserve,
 *   then capture again —, but on the ROCm 7.2 runtime the stream of the broken capture stays invalidated even after hipStreamEndCapture
 *   (every later launch on it fails): destroy it and capture on a new one.                                                              */

/* Hidden-state tap for parity tests: one sentence, writes hidden[(n_layer+1)][n_tokens][n_embd]
 * f32 (after the embedding LayerNorm and after every encoder layer, reference bert.cpp:806-901)
 * and the final embedding.  Either output may be NULL.  The tap needs every layer's normalised states, so it takes neither the
 * all-layers-in-one-launch kernel nor the folded LayerNorms: at H = 768 with BERT_HIP_LN_FOLD on (the default) its embedding
 * is that of the un-folded sequence and differs from bert_eval_batch's for the same sentence in the last bits.            */
BERT_API int32_t bert_hip_eval_hidden(struct bert_ctx *ctx, const bert_vocab_id *tokens, int32_t n_tokens,
                                      float *hidden, float *embedding);

/* Per-kernel timing with HIP events on the launch stream.  While enabled every kernel launch of
 * the forward pass carries an event pair (hipExtLaunchKernelGGL start / stop events: a timed launch runs behind system-scope
 * fences and reads up to 8 % long for sub-millisecond kernels, so never enable it inside a throughput measurement).  bert_hip_profile_report writes one line per
 * kernel: "<name> <launches> <total_ms> <flops_per_launch_avg>\n" and returns the number of bytes
 * it needed (excluding NUL); it synchronises the device first and resets the counters.  While enabled, calls on a capturing stream are
 * refused (STREAM CAPTURE AND GRAPHS above).  Behind the kernels it lists which
 * mat-mul kernel family served the weight GEMMs of the pass: "family:gemm256_f16" / "family:gemm256_q4" (256 x 256 tiles, f16
 * image / 4-bit planes dequantised in the tile load), "family:gemm_mfma_f16" / "_q4" (128 x 128 tiles), "family:gemm_naive",
 * each "<name> <launches> 0 0".  With bert_hip_set_option("profile_replay", "<kernel>:<K>") a pass runs untimed and the
 * first launch of <kernel> is followed by K repeats of itself between ONE event pair (the pair's cost spread over K launches;
 * in-place kernels then run on their own output: such a pass's results are not to be used); "" restores a pair per launch. */
BERT_API void    bert_hip_profile_enable(struct bert_ctx *ctx, int32_t on);
BERT_API int32_t bert_hip_profile_report(struct bert_ctx *ctx, char *buf, int32_t buf_len);

/* Environment, read by bert_load_from_file (eleven switches):
 *   BERT_HIP_DEVICES       "all" or a comma-separated list of HIP ordinals without repeats: the GPUs of the context
 *                          (default: the calling thread's current device — one context, one GPU, unless asked otherwise);
 *                          BERT_HIP_DEVICE=<n>, the spelling of the first builds, is read as a list of one when this is unset
 *   BERT_HIP_KERNELS       "fused" (default): two launches per layer where the shape allows it — projection + attention of a
 *                          128-slot window (qkv_attention2.hip), everything behind the attention (layer_tail.hip) —, tiled kernels
 *                          elsewhere | "tiled": GEMM, attention and LayerNorm kernels only (Q|K|V and the intermediate through
 *                          HBM).  ("naive" — the generic kernels the parity tests compare against — is a route of libbert_test.so only;
 *                          libbert.so prints a note and ignores it.)
 *   BERT_HIP_Q4            "expand" (default) | "fused" — q4_0 / q4_1 weight matrices are expanded to f16 images in HBM once
 *                          at load, or stay 4-bit in HBM and are dequantised in the tile loads of the same kernels (same values,
 *                          same bits on the fused kernels; a quarter of the weight bytes)
 *   BERT_HIP_LATENCY       1 (default) | 0 | n — calls of at most n tokens (default 768: one sentence per call, the reference's callers,
 *                          and the small batches of a polling server) take the latency route: every mat-mul of a layer split by
 *                          output features and token blocks over many workgroups (skinny.hip); same bits as the batch route
 *                          (220 us per 128-token sentence, 330 us for 16 sentences of 25 tokens, host to host)
 *   BERT_HIP_F32           "exact" (default) | "f16" — f32 model files run in f32 arithmetic like the reference's (f32 activations,
 *                          v_mfma_f32_32x32x2_f32: f32_route.hip), or with their matrices rounded to f16 through the f16 kernels
 *   BERT_HIP_WINDOW_SLOTS  16 (default) | 8 — PROCESS-WIDE: sentences start at multiples of this many slots inside the 128-slot windows of the
 *                          fused attention kernels.  8 packs mean-25-token batches into about an eighth fewer windows; the price is
 *                          that a sentence's embedding then depends, in its last bits, on where it sits in its window — 16 slots are
 *                          one k-step of the P.V MFMAs, 8 are not (tools/ubench/mfma_shift.hip) — so "the same sentence gives the
 *                          same bits in any batch" holds only with 16.  Cosines against the CPU are unchanged.
 *   BERT_HIP_CHUNK_TOKENS  max tokens evaluated per device pass by the host API (default 262144)
 *   BERT_HIP_LN_FOLD       1 (default) | 0 — models on the 256 x 256-tile mat-mul route (H = 768): the LayerNorms folded into the mat-muls around
 *                          them (no LayerNorm launch but the last; roundings differ from the un-folded sequence in the last bits), or a
 *                          LayerNorm kernel per LayerNorm.  Read at load: 0 builds no folded weight images, and set_option("ln_fold",
 *                          "1") on such a context is ignored.  bert_hip_eval_hidden always takes the un-folded sequence.
 *   BERT_HIP_POOLING       "mean" (default) | "cls" — what a sentence's embedding is made of: the mean over its tokens' final states (the
 *                          reference's; the all-MiniLM, e5 and gte families), or the final state of its FIRST token as the caller gave
 *                          it (the BGE family: bert_tokenize puts [CLS] there, the packed entry points take whatever id comes first)
 *   BERT_HIP_NORMALIZE     1 (default) | 0 — that row divided by its L2 norm (no epsilon), or as it is.  "cls" with 0 is the stored state
 *                          exactly (the f16 values converted to f32; the f32 values on the f32 route), "mean" with 0 the sums that 1
 *                          scales.  Both settings are per context and change nothing else: the same kernels run, the length guard
 *                          (NaN row, status word) and "the same sentence gives the same bits in any batch, on the latency and the batch
 *                          route, with one launch or two" hold in every mode, and whatever returns or consumes a context's embeddings
 *                          follows them — bert_eval[_batch], bert_encode[_batch], bert_hip_eval_packed[_device, _gather], the embedding
 *                          of bert_hip_eval_hidden, bert_hip_index_add_texts and _search_texts.  Any other value: a line on stderr, the
 *                          setting stays as it was (the keys below likewise).  A pass reads both once, at its start; a host call cut
 *                          into chunks or spread over devices uses one value throughout
 *   BERT_HIP_QUIET         1 = no progress text on stdout during load, no "unknown token" lines on stderr from bert_tokenize
 * bert_hip_set_option (after load; tests and tuning): "qkv2" / "tail" / "gemm256" / "latency" = "0" | "1" switch single kernels
 * of the fused family, "one_launch" = "0" | "1" (default: all layers in one launch for well-filled windows) | "2" (whenever the
 * kernel takes the batch), "gemm" / "attn" = "mfma" | "naive" (libbert_test.so), "ln_fold" = "0" | "1", "f32" = "exact" | "f16", "latency_tokens" = n, "window_slots" = "16" | "8" (process-wide default, read once
 * per forward pass), "chunk_tokens" = n, "gather_super_tokens" = n (bert_hip_eval_packed_gather: tokens per device and super-batch, 0 =
 * four device chunks), "stage_kernel" = "0" | "1" (host API: staged blocks of at most 256 KiB travel by a kernel that reads the mapped
 * pinned memory instead of the copy engine), "sparse_index_qb" = n (tuning: queries per workgroup tile of the sparse index's scan, 1 .. 8;
 * "0" = the built-in choice; a result's bits do not depend on it; set it before bert_hip_sparse_index_reserve), "sparse_index_segment_rows" = n
 * (tuning: rows per segment of a sparse index's postings, 256 .. 16384 in multiples of 256; "0" = the built-in choice; read by
 * bert_hip_sparse_index_invert; a result's bits do not depend on it), "hybrid_chunk_queries" = n (tuning: queries
 * per internal chunk of a hybrid search, 1 .. 4096, never more than the score workspace's bound allows; "0" = what that bound gives; a
 * result's bits do not depend on it), "token_index_slices" = n (tuning: slices of documents a token index's scan is cut into, 1 .. 4096,
 * never more than documents; "0" = planned; a result's bits do not depend on it; set it before bert_hip_token_index_reserve),
 * "maxsim_launch_pairs" = n (tuning and tests: pairs per launch of MaxSim's kernel, which bert_hip_maxsim[_device] and a token index's
 * rescore enqueue, 1 .. 8388608 = 2^23; a larger value is clamped to 2^23, "0" = 2^23; a result's bits do not depend on it),
 * "profile_replay" (above), "pooling" = "mean" | "cls", "normalize" = "1" | "0"
 * (BERT_HIP_POOLING / BERT_HIP_NORMALIZE above; bert_hip_pooling / bert_hip_normalize return what is in force).                       */
BERT_API void bert_hip_set_option(struct bert_ctx *ctx, const char *key, const char *value);

/* LONG TEXTS.  bert_tokenize truncates at n_max_tokens (leaving room for one [SEP]), and so does every text entry point above: what
 * lies behind the cut never reaches the model.  The entry points below embed a text of any length: it is cut into overlapping
 * windows, every window is evaluated as an ordinary sentence, and the windows' embeddings are combined into ONE row per text on the
 * device.  Nothing above changes its behaviour or its bits.
 *
 * Grouped pooling, the primitive: a packed batch plus a partition of its sentences into consecutive groups gives one embedding per
 * group.  Sentences group_cu[g] .. group_cu[g + 1] - 1 form group g; group_cu[0] = 0, group_cu[n_groups] = n_sentences, no empty group.
 *   Definition.  Let the context's settings be "pooling" and "normalize", and r_s sentence s's row as the pass gives it under the
 *   same "pooling" with "normalize" = 0 (the mean over the sentence's tokens, or its first token's state).  The weight of sentence s
 *   is w_s = cu[s + 1] - cu[s], its token count, under mean pooling and w_s = 1 under cls pooling.  The group's row is
 *   a = (sum_s w_s r_s) / sum_s w_s — for mean pooling the mean over every token state of every sentence of the group — and with
 *   "normalize" = 1 it is divided by its L2 norm (no epsilon).
 *   Arithmetic.  The ordinary forward pass runs with the raw mode handed in as an argument: the context's options are not touched, a
 *   later ordinary call and bert_hip_normalize see what they saw before.  The raw rows are f32; one workgroup per group walks its
 *   sentences in ascending order with one fused multiply-add chain per element, sum w in integers, one multiplication by
 *   1 / sum w, then the norm in the reduction order of the ordinary pooling.  No atomics: a group's bits depend on its own sentences
 *   alone — not on the other groups, the number of devices or BERT_HIP_CHUNK_TOKENS.  A group of ONE sentence takes its row
 *   unchanged, so it is, bit for bit, the embedding bert_hip_eval_packed gives that sentence, in all four modes, on the f16 and
 *   the f32 route.
 *   Memory.  The raw rows live in a grow-only [n_sentences][n_embd] f32 buffer of the engine: the first call at a new largest shape
 *   allocates (synchronises the device, illegal under stream capture) — call once at the largest shape before a capture, as for
 *   bert_hip_reserve, which does not size this buffer.  On a one-device context the raw rows never leave the device; on a
 *   multi-device context they come through the sharded host path and are pooled on the first device.
 *   eval_packed_grouped         host buffers, blocking.  group_cu is checked before anything is launched: -2, a line on stderr and
 *                               outputs untouched unless it starts at 0, ends at n_sentences and increases strictly.  Otherwise
 *                               the results and errors of bert_hip_eval_packed.  embeddings: [n_groups][n_embd].
 *   eval_packed_grouped_device  everything in HBM on the first device, enqueued on `stream`, the rules of
 *                               bert_hip_eval_packed_device.  group_cu is validated on the device: a group that is empty, not
 *                               ascending or outside [0, n_sentences] gets a NaN row and sets the status word bert_hip_check
 *                               returns, as a broken max_len does; a sentence that broke max_len (a NaN row) makes its group's row
 *                               NaN.  d_embeddings must not overlap the other buffers.
 *   The launch is listed as "group_pool" by bert_hip_profile_report.                                                             */
BERT_API int32_t bert_hip_eval_packed_grouped(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens,
                                              int32_t n_sentences, const int32_t *group_cu, int32_t n_groups, float *embeddings);
BERT_API int32_t bert_hip_eval_packed_grouped_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                                     int32_t n_sentences, int32_t n_tokens_total, int32_t max_len,
                                                     const int32_t *d_group_cu, int32_t n_groups, float *d_embeddings, void *stream);

/* All ids of a text, [CLS] ... [SEP], WITHOUT truncation (host only; tokenizer-only contexts too): returns their number n and writes
 * them to tokens iff cap >= n (tokens may be NULL with cap 0: a count).  A text of b bytes yields at most b + 2 ids.  For a text that
 * fits n_max_tokens the ids are bert_tokenize's.  Negative on an error.                                                             */
BERT_API int32_t bert_hip_tokenize_long(struct bert_ctx *ctx, const char *text, bert_vocab_id *tokens, int32_t cap);

/* The windows of a text of n_tokens ids (pure; no context).  `window` counts ALL ids of a window, its [CLS] and [SEP] included;
 * `stride` counts inner ids.  Limits: n_tokens >= 2, window >= 3 (the text entry points: <= n_max_tokens), 1 <= stride <= window - 2;
 * -2 otherwise.  Let m = n_tokens - 2 inner ids and c = window - 2.  n_tokens <= window: one window, the text itself.  Otherwise
 * windows start at inner offsets 0, stride, 2 stride, ... for as long as start + c < m, and one last window starts at m - c: every
 * window of a long text has exactly `window` ids, the first starts at the text's start, the last ends at its end, every inner id is
 * in at least one, and there are 1 + ceil((m - c) / stride) of them.  Window i is the text's first id ([CLS]), the c inner ids from
 * starts[i] (ids[1 + starts[i]] onwards), then the text's last id ([SEP]).  Returns the number of windows; writes starts[0 .. count)
 * iff cap >= count (starts may be NULL with cap 0: a count).                                                                      */
BERT_API int32_t bert_hip_plan_windows(int32_t n_tokens, int32_t window, int32_t stride, int32_t *starts, int32_t cap);

/* bert_hip_encode_batch for texts of any length: per text tokenize_long, plan_windows, every window an ordinary sentence, one group
 * per text, grouped pooling (above: under mean pooling a text's row is the token-weighted mean over its windows' tokens — tokens
 * in an overlap count once per window that holds them —, normalised or not as the context says).  A text that fits its window is one
 * group of one sentence: its embedding is, bit for bit, bert_encode_batch's.  Texts are tokenized on up to n_threads host threads, the
 * id buffer of a text sized from its byte length; they go to the engine in groups of at most 16384 windows, a text's windows never
 * in two groups (a text with more windows is a group of its own).  n_windows (nullable): [n_inputs], the number of windows of every
 * encoded text.  Returns the number of inputs encoded (all of them, or those in front of the first failed group — later embeddings
 * stay untouched), -1 for a context without a device, -2 with the outputs untouched for a window or stride outside the limits of
 * bert_hip_plan_windows and 3 <= window <= n_max_tokens.  A row's bits do not depend on the other texts of the call.               */
BERT_API int32_t bert_hip_encode_long_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, int32_t window,
                                            int32_t stride, float **embeddings, int32_t *n_windows);

/* TOKEN ROWS AND LATE INTERACTION.  Everything above returns one row per sentence or per text; the final state of every token is
 * computed on every pass and then dropped.  The entry points below return those states — per-token embeddings, the input of BERTScore
 * and of ColBERT-style late-interaction scoring — and score two sets of them by MaxSim on the device.  Nothing above changes its
 * behaviour or its bits.
 *
 * Token rows.  A pass with one more destination: rows[t] is the final state (after the last layer's output LayerNorm) of token t of
 * the packed batch, n_embd values, in the order of `tokens`.
 *   Route.  Such a pass does not take the all-layers-in-one-launch kernel (that kernel pools inside the launch and leaves no row-order
 *   copy of the states); it runs the latency route, the fused two-launches-per-layer route, the folded-LayerNorm route or the f32 route
 *   as a call without the rows would with "one_launch" = "0".  Unlike bert_hip_eval_hidden, LayerNorm folding stays as planned, so the
 *   call's embeddings are, bit for bit, bert_hip_eval_packed's, and a sentence's rows have the same bits alone and in any batch.
 *   flags.  bit 0 (1): every row divided by its own L2 norm — the sum of squares in f32, a lane's elements in ascending order, then the
 *   lanes in the butterfly order of the pooling's reductions, 1 / sqrt, no epsilon (a zero row gives NaN, as in the pooling).  bit 1
 *   (2, device form only): rows are f16, rounded to nearest even, instead of f32.  Without bit 0 the f32 rows are the stored states
 *   exactly: the f16 values converted to f32, or the f32 values on the f32 route.  Under "pooling" = "cls", "normalize" = "0" the
 *   un-normalised row of a sentence's first token is that sentence's embedding, bit for bit.
 *   Guard.  The tokens of a sentence that is empty or longer than max_len get NaN rows (and the sentence a NaN embedding and the status
 *   word of bert_hip_check, as in every device call).
 *   The copy is one launch behind the pooling launch, listed as "token_rows" by bert_hip_profile_report; it allocates nothing, so a
 *   context sized by bert_hip_reserve may call the device form under stream capture.
 *   eval_packed_tokens_device  the rules of bert_hip_eval_packed_device (everything in HBM on the first device, enqueued on `stream`).
 *                              d_rows: [n_tokens_total][n_embd] f32, or f16 with flags bit 1; d_embeddings: [n_sentences][n_embd] f32 or
 *                              NULL (the embeddings then stay in the engine's workspace).  The buffers must not overlap.
 *   eval_packed_tokens         host buffers, blocking, on the context's FIRST device (a multi-device context does not spread it).
 *                              flags: bit 0 only; rows [cu_seqlens[n_sentences]][n_embd] f32; embeddings [n_sentences][n_embd] or NULL.
 *                              The batch is cut at BERT_HIP_CHUNK_TOKENS between sentences, one plain copy per chunk and direction (not
 *                              the pipelined staging of bert_hip_eval_packed); the cut does not show in the bits.  0; -1 without a device;
 *                              -2 with the outputs untouched after a line on stderr for a sentence that cannot be evaluated; -3 on a device error.
 *   encode_tokens_batch        texts: tokenized as bert_encode_batch does (same truncation), on up to n_threads host threads.  cu_out
 *                              [n_inputs + 1] receives the cumulative token counts, always.  Returns the total token count; writes rows
 *                              [total][n_embd] iff rows != NULL and cap_rows >= that count (rows NULL with cap_rows 0: a count call that
 *                              only tokenizes).  flags: bit 0 only.  Negative on an error (-1 without a device).
 *
 * MaxSim.  Q [nq_tokens][H] and D [nd_tokens][H] are two packed sets of token rows with cumulative lengths qcu [n_q + 1] and dcu
 * [n_d + 1] (sentence a of Q is rows qcu[a] .. qcu[a + 1] - 1).  For a pair (a, b)
 *       score(a, b) = sum over the tokens i of a of ( max over the tokens j of b of <Q_i, D_j> ),
 * divided by (float)len(a) with mode bit 0.  pairs NULL: all pairs, scores [n_q][n_d]; else pairs [n_pairs][2] of (a, b), in any order
 * and with repeats, scores [n_pairs].  H: a multiple of 8 from 8 to 1024 (rows are whole 16-byte pieces), else -2.
 *   Arithmetic.  The rows are f16.  Every inner product is the chain of the f16 index (v_mfma_f32_32x32x16_f16, f32 accumulation, k
 *   ascending; at H % 16 == 8 the last half step is zero-filled in registers).  The max is exact.  The sum runs in one fixed order:
 *   the query tokens in blocks of 32, a block's 32 maxima (a short last block padded with +0) added in the butterfly order of the
 *   pooling's wave reduction, the blocks' sums added in ascending order; the mean is one division.  No atomics: a pair's bits depend
 *   on its own rows alone — not on its place in the output, the other pairs, or the list form against the all-pairs form.
 *   Masking.  Rows outside a pair's two ranges are never read into its score: a document slot behind len(b) enters the max as -inf
 *   (a pair whose similarities are all negative scores negative), a query slot behind len(a) adds 0.
 *   maxsim_device   rows (f16, 16-byte aligned), lengths, pairs and scores in HBM on the first device, enqueued on `stream`; allocates
 *                   nothing; listed as "maxsim" by bert_hip_profile_report.  The lengths and pairs are checked on the device: a pair
 *                   whose index lies outside [0, n_q) x [0, n_d), or one of whose sentences is empty, descends in its cu entries or
 *                   starts below 0, gets a NaN score; its neighbours are untouched.  -2 for a bad H, count or pointer.
 *   Limits.         n_pairs < 2^31 with a pair list, n_q n_d < 2^31 without, and every one of those pairs is scored: one workgroup
 *                   serves one pair, and a call of more than 2^23 pairs is enqueued as several launches of at most 2^23 (one kernel
 *                   node each in a captured graph, and no sample of bert_hip_profile_report, which times single launches; the tuning
 *                   key "maxsim_launch_pairs" lowers that number).  The host form takes sets
 *                   of at most 2^31 values (tokens x H) each, -2 beyond; bert_hip_eval_packed_tokens_device at most 2^25 tokens, -2
 *                   beyond.
 *   maxsim          host buffers, blocking: f32 rows, uploaded and rounded to f16 (nearest even) on the device, then maxsim_device.
 *                   Everything is validated first — cu entries strictly ascending from an entry >= 0, every pair in range —: -2 after a
 *                   line on stderr with the scores untouched.  -1 without a device, -3 on a device error.                          */
BERT_API int32_t bert_hip_eval_packed_tokens_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                                    int32_t n_sentences, int32_t n_tokens_total, int32_t max_len, int32_t flags,
                                                    void *d_rows, float *d_embeddings, void *stream);
BERT_API int32_t bert_hip_eval_packed_tokens(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens,
                                             int32_t n_sentences, int32_t flags, float *rows, float *embeddings);
BERT_API int64_t bert_hip_encode_tokens_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n_inputs, const char **texts, int32_t flags,
                                              int32_t *cu_out, float *rows, int64_t cap_rows);
BERT_API int32_t bert_hip_maxsim_device(struct bert_ctx *ctx, const void *d_q, const int32_t *d_qcu, int32_t n_q, const void *d_d,
                                        const int32_t *d_dcu, int32_t n_d, int32_t H, const int32_t *d_pairs, int32_t n_pairs, int32_t mode,
                                        float *d_scores, void *stream);
BERT_API int32_t bert_hip_maxsim(struct bert_ctx *ctx, const float *q, const int32_t *qcu, int32_t n_q, const float *d, const int32_t *dcu,
                                 int32_t n_d, int32_t H, const int32_t *pairs, int32_t n_pairs, int32_t mode, float *scores);

/* SENTENCE PAIRS AND SCORES.  A cross-encoder reads a query and a document as ONE sentence, [CLS] a [SEP] b [SEP], with token type 0 on
 * the first segment and 1 on the second, and ends in a classification head: logits = Wc tanh(Wp h_CLS + bp) + bc, h_CLS the
 * un-normalised final state of [CLS] (HuggingFace BertForSequenceClassification; cross-encoder/ms-marco-MiniLM-L-6-v2 is one, with the
 * geometry of the MiniLM bi-encoders).  Nothing above changes its behaviour or its bits.
 *
 * The model file.  Four optional tensors behind the encoder's set, all or none: pooler.dense.weight [n_embd, n_embd], pooler.dense.bias
 * [n_embd], classifier.weight [n_embd, n_labels], classifier.bias [n_labels] (ne0 = in-features; 2-D tensors in the file's type, 1-D
 * in f32; 1 <= n_labels <= 8).  bert_hip_n_labels: the labels of the context's head, 0 without one.
 *
 * Token types.  first_len[b] is the number of leading tokens of sentence b that take row 0 of the token-type table; every token at a
 * place at or behind it takes row 1.  first_len NULL: row 0 everywhere, and then a typed call returns the untyped call's bits.  The
 * host forms want 0 <= first_len[b] <= the sentence's length (-2 otherwise); the device forms take any value (<= 0: all row 1; >= the
 * length: all row 0).  A typed pass plans and runs like any other pass; only its embedding launch differs.
 *   eval_packed_typed[_device]  bert_hip_eval_packed[_device] with types: the context's pooling, normalisation and routes.  For any BERT
 *                               that was trained with segments.
 *
 * Scores.  score_packed[_device] run a typed pass that ends in the [CLS] rows and launch the head on them ("cls_head" in
 * bert_hip_profile_report): scores [n_sentences][n_labels] f32.  flags 0: the logits; 1: 1 / (1 + exp(-logit)) per label (what
 * sentence-transformers' CrossEncoder applies for n_labels == 1).  The context's "pooling" / "normalize" do not enter.  The head runs
 * on the matrix cores for n_embd % 8 == 0, n_embd <= 1024 — the [CLS] rows and Wp rounded to f16, f32 accumulation — and in plain f32
 * for f32 files on the f32 route and any other n_embd.  Its sums run in one fixed order without atomics: a pair's scores have the same
 * bits alone, anywhere in a batch and in any batch size.  -2 after a line on stderr, nothing written, for a model without a head.
 *   *_device   the rules of bert_hip_eval_packed_device: everything in HBM on the first device, enqueued on `stream`; after
 *              bert_hip_reserve they allocate nothing and may be captured into a graph.
 *   host forms blocking, on the context's FIRST device (a multi-device context does not spread these calls).  Cut at
 *              BERT_HIP_CHUNK_TOKENS between sentences, one plain copy per chunk and direction.  0; -1 without a device; -2 with the
 *              outputs untouched for a sentence that cannot be evaluated or a first_len outside [0, length]; -3 on a device error.
 *
 * Pairs of texts.
 *   tokenize_pair  a is tokenized as bert_tokenize does, [CLS] .. [SEP]; b likewise, losing its [CLS]; tokens = a's ids, then b's;
 *                  *first_len = the count of a's ids.  When the two exceed n_max_tokens (>= 4; tokens must hold that many), a is cut
 *                  to at most n_max_tokens / 2 ids and b to the remainder, each cut keeping its [SEP] last.  Works on tokenizer-only
 *                  contexts.  0, or -2 for a bad argument.
 *   score_pairs    both sides tokenized on up to n_threads host threads, paired by tokenize_pair's rule at the model's n_max_tokens,
 *                  packed and scored: scores [n_pairs][n_labels].  Returns the number of pairs scored (bert_hip_encode_batch's
 *                  conventions: it stops at the first failure, later outputs untouched), -1 without a device, -2 without a head.   */
BERT_API int32_t bert_hip_n_labels(struct bert_ctx *ctx);
/* RELATIVE POSITION BIAS (MPNet: sentence-transformers/all-mpnet-base-v2, multi-qa-mpnet-base-*).  One optional tensor behind the
 * encoder's set, encoder.relative_attention_bias.weight [n_head, 32] (ne0 = n_head: HuggingFace's [32][n_head]), f32 or f16 and never
 * quantised; it may stand beside either head.  With it every attention score of every layer is
 *     <q_i, k_j> / sqrt(d_head) + W[bucket(j - i)][head],
 * bucket as MPNetEncoder.relative_position_bucket with 32 buckets and max_distance 128.  Any other bucket count fails the load.  Such a
 * model runs the layered, the LayerNorm-folding or the f32 route (the add lives in the attention launch; the fused projection +
 * attention kernel, the one-launch kernel and the latency route are not taken); everything behind the encoder serves it unchanged.
 * Its texts are wrapped in the ids of <s> and </s> of the file's vocabulary instead of 101 / 102 (a load error if either is absent;
 * a file without the tensor keeps 101 / 102 whatever its vocabulary holds), and bert_hip_score_pairs refuses it with -2: MPNet lays a
 * pair out differently; the packed and typed entry points take ids as given.  ggml_file.hf_mpnet_weights converts a checkpoint:
 * position rows from 2 on, a zero token-type table.
 *   relative_attention  1 if the context's model file has the tensor (tokenizer-only contexts included), 0 if not, -1 without a context. */
BERT_API int32_t bert_hip_relative_attention(struct bert_ctx *ctx);
BERT_API int32_t bert_hip_tokenize_pair(struct bert_ctx *ctx, const char *text_a, const char *text_b, bert_vocab_id *tokens, int32_t *n_tokens,
                                        int32_t *first_len, int32_t n_max_tokens);
BERT_API int32_t bert_hip_eval_packed_typed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, const int32_t *first_len,
                                            int32_t n_sentences, float *embeddings);
BERT_API int32_t bert_hip_eval_packed_typed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                                   const int32_t *d_first_len, int32_t n_sentences, int32_t n_tokens_total, int32_t max_len,
                                                   float *d_embeddings, void *stream);
BERT_API int32_t bert_hip_score_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, const int32_t *first_len,
                                       int32_t n_sentences, int32_t flags, float *scores);
BERT_API int32_t bert_hip_score_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                              const int32_t *d_first_len, int32_t n_sentences, int32_t n_tokens_total, int32_t max_len,
                                              int32_t flags, float *d_scores, void *stream);
BERT_API int32_t bert_hip_score_pairs(struct bert_ctx *ctx, int32_t n_threads, int32_t n_pairs, const char **texts_a, const char **texts_b,
                                      int32_t flags, float *scores);

/* LEARNED SPARSE EMBEDDINGS.  A BERT with its masked-language-model head (HuggingFace BertForMaskedLM; the SPLADE family is trained this
 * way) turns a text into one non-negative weight per vocabulary entry,
 *     w[v] = max over the text's tokens i of log(1 + relu(logit[i][v])),   logit[i] = E t_i + bias,   t = LayerNorm(gelu(Wt x + bt)),
 * x the final states of the pass, E the word-embedding matrix (the decoder is tied to it).  [CLS] and [SEP] take part, as under
 * HuggingFace's attention mask.  Nothing above changes its behaviour or its bits.
 *
 * The model file.  Five optional tensors behind the encoder's set and the classification head (the two heads are independent), all or
 * none: cls.predictions.transform.dense.weight [n_embd, n_embd] (the file's type), cls.predictions.transform.dense.bias,
 * cls.predictions.transform.LayerNorm.weight, .LayerNorm.bias [n_embd] and cls.predictions.bias [n_vocab] (f32).  The decoder matrix is
 * not stored.  bert_hip_has_mlm_head: 1 if the context's model has the head, else 0.
 *
 * What is computed.  out[b][v] = z > 0 ? log1pf(z) : +0 with z = (max over the tokens of sentence b of <t_i, E_v>) + bias[v]: log1p and
 * relu are monotone, so the max moves inside and the bias is added once.  For n_embd % 8 == 0, n_embd <= 1024 the products run on the
 * matrix cores: t and E as f16 (E: the file's f16 bits, or its f32 / q4 values rounded once), f32 accumulation, the index's chain; for
 * f32 files on the f32 route and any other n_embd in plain f32.  The logits [tokens][n_vocab] never reach memory: the max over a
 * sentence's tokens is taken in registers and only [n_sentences][n_vocab] leaves the chip.  The max is exact, so a sentence's weights
 * have the same bits alone, anywhere in a batch, in any batch size and from run to run.  The context's "pooling" / "normalize" do not
 * enter.  The launches are "mlm_transform", "mlm_layernorm", "sparse_vocab", "sparse_finish" and "sparse_topk" in
 * bert_hip_profile_report.
 *   sparse_packed[_device]       weights [n_sentences][n_vocab] f32, dense.
 *   sparse_topk_packed[_device]  per sentence the k largest POSITIVE weights (1 <= k <= 256) with their vocabulary ids, larger first,
 *                                equal weights smaller id first: ids [n_sentences][k] i32, weights [n_sentences][k] f32; a sentence with
 *                                fewer than k positive weights ends in ids of -1 with weights +0.  The dense rows behind it live in a
 *                                scratch of at most 32 MiB: the head runs in chunks of sentences, the chunk fixed at bert_hip_reserve.
 *   *_device   the rules of bert_hip_eval_packed_device: everything in HBM on the first device, enqueued on `stream`; after
 *              bert_hip_reserve (which accounts for the transform's buffer and the scratch) they allocate nothing and may be captured
 *              into a graph.
 *   host forms blocking, on the context's FIRST device.  Cut at BERT_HIP_CHUNK_TOKENS between sentences, one plain copy per chunk and
 *              direction.  0; -1 without a device; -2 after a line on stderr, the outputs untouched, for a model without the head, a k
 *              outside its range or a sentence that cannot be evaluated; -3 on a device error.
 *   encode_sparse_batch  texts tokenized on up to n_threads host threads as bert_hip_encode_batch does, packed, top-k: returns the number
 *              of texts encoded (it stops at the first failure, later outputs untouched), -1 without a device, -2 as above.            */
BERT_API int32_t bert_hip_has_mlm_head(struct bert_ctx *ctx);
BERT_API int32_t bert_hip_sparse_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences,
                                        float *weights);
BERT_API int32_t bert_hip_sparse_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                               int32_t n_sentences, int32_t n_tokens_total, int32_t max_len, float *d_weights, void *stream);
BERT_API int32_t bert_hip_sparse_topk_packed(struct bert_ctx *ctx, const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences,
                                             int32_t k, int32_t *ids, float *weights);
BERT_API int32_t bert_hip_sparse_topk_packed_device(struct bert_ctx *ctx, const bert_vocab_id *d_tokens, const int32_t *d_cu_seqlens,
                                                    int32_t n_sentences, int32_t n_tokens_total, int32_t max_len, int32_t k, int32_t *d_ids,
                                                    float *d_weights, void *stream);
BERT_API int32_t bert_hip_encode_sparse_batch(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, int32_t k, int32_t *ids,
                                              float *weights);

/* Embedding index: rows in HBM on the context's FIRST device (bert_hip_device), exact top-k search by inner product.
 * An index belongs to the context it was made from: bert_free frees any index the caller left alive.  Like every
 * entry point of a context, the index functions are not re-entrant on one context.
 *   create   dim: 0 = bert_n_embd(ctx), else 1 .. 2048.  dtype: 0 = f32 rows, 1 = f16 rows (rounded to nearest even; the
 *            queries are rounded to f16 the same way), 2 = int8 rows with one f32 scale per row (the queries quantized the
 *            same way, on the device; below), 3 = "b1": one sign bit per element and no scale (the queries quantized to int8;
 *            below).  Memory per row: 4 * ceil(dim / 8) * 8 bytes (f32), 2 * ceil(dim / 16) * 16
 *            (f16), dpad + 4 with dpad = ceil(dim / 32) * 32 (int8), dpad / 8 with dpad = ceil(dim / 128) * 128 (b1: 48 bytes
 *            at dim 384).  NULL + a message on stderr on error (tokenizer-only context, no device, bad arguments).
 *   add      appends rows [n][dim] (f32); they get ids size, size + 1, ...; returns the first new id, negative on error
 *            (index unchanged).  add_device: the rows in device memory of the index's device, enqueued on `stream`.
 *            add_texts: encodes the texts (dim must equal n_embd) on the context's devices as bert_hip_encode_batch does; on a
 *            single-device context the embeddings go from the forward pass's device output straight into the index.
 *   search   ids[n_queries][k] and scores[n_queries][k], best first; 0 on success, negative on error (outputs untouched).
 *            search_device: queries and results in device memory, enqueued on `stream`.  search_texts: the queries are texts,
 *            encoded like add_texts's (single device: into a device buffer, no host round trip).
 *   reserve  sizes the storage for n_rows rows and the search workspace for up to n_queries queries with any k' <= k now,
 *            so that the *_device calls within those bounds never allocate (allocation synchronises the device: illegal under
 *            stream capture).  Without it storage and workspace grow on demand.
 * Semantics:
 *   - score = sum_i q[i] * row[i], accumulated in f32: f32 rows on v_mfma_f32_32x32x2_f32 (an f32 fma chain), f16 rows and
 *     f16-rounded queries on v_mfma_f32_32x32x16_f16 (rows zero-padded to its k-step, which changes no sum).  With "normalize" = 1
 *     (the default) the engine's embeddings are L2-normalised: for them the score is the cosine; with 0 it is the plain inner
 *     product of what add_texts and search_texts encoded.
 *   - int8 (dtype 2), all arithmetic f32 unless stated: each row and each query x is quantized on its own, amax = max_i |x_i|,
 *     scale = amax / 127 (correctly rounded), code_i = clamp(rint(x_i / scale), -127, 127) (rint: nearest even; the division
 *     correctly rounded), every code 0 if scale == 0; if any x_i is NaN or +-inf the scale is NaN and every code 0.  Codes
 *     are zero-padded to dpad.  score = ((float)dot * qscale) * rscale in that order (two roundings, no fma), where
 *     dot = sum_i qcode_i * rcode_i is an exact int32 converted with round-to-nearest-even.  So a row holding a NaN OR an inf
 *     scores NaN and is never returned (an f32 index can return a row holding an inf); a query holding one returns only
 *     id -1 / -INFINITY slots; a zero query scores 0 against every finite row.  The same determinism as below holds.
 *   - 1-bit (dtype 3, "b1"; asymmetric: bit rows, int8 queries): element i of a row is bit i & 31 of little-endian u32 word
 *     i >> 5, set iff x_i > 0 as an IEEE f32 comparison — so -0, NaN and -inf give 0 and +inf gives 1.  Unlike int8, non-finite
 *     elements of a ROW are not detected: such a row is stored and returned like any other.  Rows are padded with zero bits
 *     to dpad = ceil(dim / 128) * 128 elements (whole 16-byte pieces); there is no row scale.  Queries are quantized exactly as
 *     for int8 (scale = amax / 127, code_i = clamp(rint(x_i / scale), -127, 127), a NaN scale and zero codes for a non-finite
 *     element), the codes zero-padded to this dpad.  score = (float)dot * qscale, where dot = sum_i qcode_i * (bit_i ? +1 : -1)
 *     is an exact int32 (the padding meets zero codes).  A query holding a NaN or an inf returns only id -1 / -INFINITY slots;
 *     a zero query scores +0 against every row, so the smallest ids win.  Equal scores are common with this form: the order
 *     rule below decides every one.  The same determinism as below holds.  Meant as the coarse stage of search_rescored.
 *   - order: larger score first; equal scores (==, so +0 equals -0) smaller id first.  Rows with a NaN score are never
 *     returned.  Slots beyond the rows that can be returned are id -1, score -INFINITY.  An empty index is valid.
 *   - 1 <= k <= 256, anything else is an error; n_queries == 0 is a successful no-op; large n_queries run in internal chunks.
 *   - a row's score for a query has the same bits whatever the other queries of the call, the number of add calls that built
 *     the index, reserved or grown storage, k (top-10 is the first 10 entries of top-100), and host or device entry point.
 *   - *_device calls are asynchronous on the caller's stream; an index has ONE event, so its eagerly enqueued operations never
 *     overlap, whatever streams they were enqueued on.  Captured calls and graph launches: STREAM CAPTURE AND GRAPHS above.
 * Removing rows, filtered search, compaction, files:
 *   remove   marks rows as deleted.  Ids are stable: the other rows keep theirs, new rows still get size, size + 1, ... (size
 *            counts removed rows too).  A removed row is never returned by any search (search, search_device, search_texts
 *            and the filtered forms).  ids out of [0, size): error, index unchanged.  Repeats and already-removed ids are
 *            ignored.  Returns the number of rows newly removed.  Blocking.  n_live: size minus removed rows; -1 without
 *            an index.  From the first removal on the index keeps one bit per row on the device (sized with the rows by
 *            reserve), so add_device stays free of allocations and host copies within the reserved bounds.
 *   search_filtered   a search with an allow-list shared by all queries of the call: allow[w] bit b set = row 32 w + b may
 *            be returned.  n_words >= ceil(size / 32) or error (-2); bits at and beyond size are ignored; allow == NULL =
 *            all rows (then n_words is ignored) and the call is bert_hip_index_search.  Everything the search block above
 *            promises holds over the rows that are live AND allowed: the same score bits as an unfiltered search, the same
 *            order rule, -1 / -INFINITY slots when fewer than k rows qualify.  search_filtered_device: queries, allow-list
 *            and results in device memory, asynchronous on `stream` under the one-event rule; within the bounds of reserve
 *            it never allocates.  Blocks of 32 rows without a qualifying row cost neither loads nor arithmetic.
 *   compact  drops the removed rows' storage.  Live rows keep their order and stored bits and get ids 0 .. n_live - 1;
 *            old_ids (NULL, or room for n_live entries) receives the former id of each new id.  Returns the new size (an
 *            index without removed rows: a no-op that returns size).  Blocking.
 *   save / load   the index as stored (format below), so a loaded index answers every search with the bits the saved one
 *            gave.  save writes path + ".tmp" and renames it; 0 or negative.  load: NULL + a line on stderr for a
 *            tokenizer-only context, an unreadable, truncated, over-long or inconsistent file; the file is checked against
 *            its header before anything is allocated.  The loaded index belongs to ctx like a created one; its dim need
 *            not be bert_n_embd(ctx).
 * Rescoring and two-stage search:
 *   rescore  scores each query against ITS OWN candidates and returns the best k of them: cand_ids[n_queries][n_cand] are row
 *            ids; works on any dtype, with the index's own score rule — for distinct ids, query q's result has the ids and
 *            the score bits of bert_hip_index_search_filtered called with that one query and an allow-list of exactly its
 *            candidates.  -1 entries and removed rows are skipped.  An id < -1 or >= size is an error (-2, nothing
 *            written) in the host call; the device call treats it as -1.  An id that appears more than once in a query's
 *            list counts as that many candidates (it can be returned more than once); lists that come from a search are
 *            distinct.  1 <= k <= 256, 1 <= n_cand <= 1024, k may exceed n_cand: slots beyond the candidates that remain are
 *            id -1 / -INFINITY.  rescore_device: queries, candidates and results in device memory, asynchronous on `stream`
 *            under the one-event rule.  The workspace ([n_queries][n_cand] entries, queries in internal chunks) is not part
 *            of reserve and grows on demand, which allocates: call once at the largest shape before a stream capture.
 *   search_rescored   a search of `coarse` with k' = n_cand, then rescore on `fine` with the same f32 queries; the candidates
 *            stay on the device between the two.  Both indexes must belong to one context and agree in dim and size (they
 *            are meant to hold the same rows in the same order, removals included: a candidate that `fine` has removed is
 *            skipped), and 1 <= k <= n_cand <= 256; otherwise -2.  The result equals the two public calls chained by hand.
 *            search_rescored_device: asynchronous on `stream`; both indexes' events are honoured.  The same advice on
 *            allocation as for rescore holds (the coarse search's workspace is covered by coarse's reserve with k = n_cand).
 * Reading rows back, cluster partition and probed search:
 *   get_rows  rows[n][dim] = the stored rows ids[0 .. n) as f32, removed rows included: the bits (f32), the exact conversion
 *            (f16), (float)code * scale with one rounding (i8; NaN for a row whose scale is NaN), +1.0 or -1.0 per bit (b1).
 *            An id outside [0, size): -2, nothing written.  Blocking.  This is "the row" of partition and kmeans below.
 *   partition   installs centroids[n_lists][dim] (host f32, every element finite or -2; 1 <= n_lists <= 65536; n_lists == 0
 *            drops the partition) and assigns every current row, removed ones included, to one list.  The rule, through
 *            public calls: the list of row r is the id that bert_hip_index_search returns with k = 1 on an f32 index that
 *            holds the centroids as rows 0 .. n_lists - 1, queried with get_rows(r) — so equal scores go to the smaller list
 *            id, by the order rule above; a row whose every score is NaN (the search returns -1) goes to list 0.  Blocking.
 *            Storage stays in id order: ids, add, remove, save and every other search are untouched, and an index without a
 *            partition launches what it always did.  n_lists: the number of lists, 0 without a partition, -1 without an
 *            index.  partition_centroids: the centroids as installed, [n_lists][dim].  partition_lists: list_of_row[size],
 *            -1 for an unassigned row; both -2 without a partition.
 *            Rows added after partition (add, add_device, add_texts) are unassigned: they form the TAIL, which every probed
 *            search scans in full; add_device does nothing for the partition, so it stays free of allocations and legal
 *            under stream capture.  partition again, with the same or new centroids, assigns everything.  remove changes
 *            nothing in the partition: the scan reads the live bits.  compact keeps the partition: each live row keeps its
 *            list under its new id, the tail stays the tail.  The index file holds no partition, and a loaded index has
 *            none: partition_save / partition_load below keep it in a file of its own (or keep partition_centroids and
 *            partition again after the load: the assignment is a deterministic function of the stored rows and the
 *            centroids, but it assigns the former tail as well).
 *   kmeans   spherical k-means over the LIVE rows as get_rows returns them; centroids[n_lists][dim]: in, the initial centroids
 *            (finite, or -2; the caller seeds them), out, the refined ones.  Each of the n_iter >= 1 iterations assigns by
 *            the rule of partition, then replaces each centroid by the f32 sum of its members divided by that sum's L2 norm;
 *            a list without a live member, or whose sum has a zero or non-finite norm, keeps its centroid.  The sums are
 *            taken in an order fixed by the members' positions (no atomics): the same input gives the same bits.  The index
 *            (its rows, its partition) is unchanged.  Blocking.
 *   search_probed   1 <= nprobe <= min(n_lists, 256), 1 <= k <= 256, no partition: -2; n_queries == 0 is a no-op.  Query q's
 *            result has the ids and the score bits of bert_hip_index_search_filtered called with that one query and an
 *            allow-list of exactly: the rows of the nprobe lists that bert_hip_index_search(k = nprobe) returns for q on the
 *            f32 index of the centroids, plus every tail row.  Removed rows are skipped; slots beyond the qualifying rows are
 *            -1 / -INFINITY.  A query holding a NaN or an inf probes no list (its centroid search returns only -1); the tail
 *            is still scanned, as the filtered search would (i8, b1: only empty slots, as always).  With nprobe == n_lists
 *            and no NaN the result equals bert_hip_index_search.  The determinism promises above hold: a query's result
 *            depends neither on the other queries, nor on k, nor on the entry point.  search_probed_device: asynchronous on
 *            `stream` under the one-event rule (the index's event and its centroid index's are both honoured); nothing
 *            leaves the device between the centroid search, the scan of the lists (only k entries per list reach HBM) and
 *            the merge.  The workspace ([n_queries][nprobe + ceil(tail / 1024)][k] entries, queries in internal chunks) is
 *            not part of reserve and grows on demand, which allocates: call once at the largest shape before a stream
 *            capture.
 *   search_probed_filtered   search_probed with the allow-list of search_filtered.  Query q's result has the ids and the score
 *            bits of bert_hip_index_search_filtered called with that one query and an allow-list of exactly: (the rows of the
 *            nprobe lists that the centroid index returns for q, plus every tail row) AND the caller's list.  allow == NULL
 *            is search_probed (n_words is ignored); n_words < ceil(size / 32): -2; bits at and beyond size are ignored and
 *            never read; argument ranges are search_probed's; removed rows, NaN queries and -1 / -INFINITY slots as stated
 *            for search_filtered and search_probed.  32 consecutive members of a list or of the tail without a qualifying
 *            row cost neither row loads nor arithmetic.  An index with removed rows but no allow-list launches what
 *            search_probed always did.  search_probed_filtered_device: queries, allow-list and results in device memory,
 *            asynchronous on `stream` under the one-event rule; it uses the workspace of search_probed_device and never
 *            allocates where a search_probed_device of the same shape has run.
 *   search_rescored_probed   search_rescored whose coarse stage is coarse's search_probed_filtered with k' = n_cand: the
 *            candidates stay on the device, then `fine` rescores them with the same f32 queries.  The result equals the two
 *            public calls chained by hand.  `coarse` must have a partition, `fine` needs none; the allow-list (NULL: none;
 *            n_words as above, against the common size) applies to the coarse stage, so no disallowed row is returned.  The
 *            conditions of search_rescored (one context, equal dim and size, 1 <= k <= n_cand <= 256) and of search_probed
 *            (nprobe) hold, otherwise -2.  search_rescored_probed_device: asynchronous on `stream`; both indexes' events
 *            are honoured; the advice on allocation of rescore and search_probed holds.
 *   partition_save / partition_load   the partition as a file of its own beside the index file (format below; the index file
 *            and its version are untouched).  save writes path + ".tmp" and renames it; -2 without a partition.  load checks
 *            the header against the file's length before anything is read or allocated, then requires dim == the index's
 *            dim, 1 <= n_lists <= 65536, n_part <= size, every centroid element finite and every list id in [0, n_lists);
 *            any failure is -2 or -3 after a line on stderr, and the index keeps the partition it had.  On success the
 *            file's centroids and lists are installed as they are: NO assignment runs (the lists are the file's even where
 *            an assignment would decide otherwise), rows at and beyond n_part are the tail, and n_lists,
 *            partition_centroids, partition_lists and every probed search give the bits the saving index gave.  Blocking.
 * Errors of the functions that take an index: -1 no index, -2 bad arguments (after a line on stderr), -3 an error of the
 * index or the device (its message on stderr), -4 an exception.  Outputs are untouched on error.
 * File format (little-endian).  Header, 64 bytes: magic "BHIPIDX1" (8 bytes), u32 version = 1, u32 dtype (0 f32, 1 f16,
 * 2 i8, 3 b1), u32 dim, u32 dpad (elements per stored row: dim rounded up to 8 (f32), 16 (f16), 32 (i8), 128 (b1: bits)), u32
 * n_rows (= size, removed rows included), u32 has_live (0 | 1), 32 zero bytes.  Then n_rows * dpad * elem_size bytes of rows
 * exactly as stored (zero-padded to dpad; elem_size 4, 2, 1; b1: n_rows * dpad / 8 bytes); for i8, n_rows f32 row scales; if has_live, ceil(n_rows / 32) u32 words,
 * bit b of word w set = row 32 w + b is live, the bits at and beyond n_rows zero.  The file is exactly that long.
 * Partition file format (little-endian).  Header, 64 bytes: magic "BHIPPRT1" (8 bytes), u32 version = 1, u32 dim, u32 n_lists,
 * u32 n_part (the number of assigned rows; the rows behind are the tail), 40 zero bytes.  Then n_lists * dim f32 centroids, then
 * n_part i32 list ids.  The file is exactly that long.                                                                    */
struct bert_hip_index;
BERT_API struct bert_hip_index *bert_hip_index_create(struct bert_ctx *ctx, int32_t dim, int32_t dtype);
BERT_API void    bert_hip_index_free(struct bert_hip_index *ix);
BERT_API int32_t bert_hip_index_size(struct bert_hip_index *ix);
BERT_API int32_t bert_hip_index_reserve(struct bert_hip_index *ix, int32_t n_rows, int32_t n_queries, int32_t k);
BERT_API int32_t bert_hip_index_add(struct bert_hip_index *ix, int32_t n, const float *rows);
BERT_API int32_t bert_hip_index_add_device(struct bert_hip_index *ix, int32_t n, const float *d_rows, void *stream);
BERT_API int32_t bert_hip_index_add_texts(struct bert_hip_index *ix, int32_t n_threads, int32_t n, const char **texts);
/* add_texts for texts of any length (LONG TEXTS above: bert_hip_encode_long_batch's rows, one per text): returns the first new id, -2
 * for a bad window or stride, negative on any error with the index at its old size.  Single device: the pooled rows go from the
 * device buffer straight into the index; several: through the host.                                                            */
BERT_API int32_t bert_hip_index_add_long_texts(struct bert_hip_index *ix, int32_t n_threads, int32_t n, const char **texts, int32_t window,
                                               int32_t stride);
BERT_API int32_t bert_hip_index_search(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t k,
                                       int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_search_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t k,
                                              int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_search_texts(struct bert_hip_index *ix, int32_t n_threads, int32_t n_queries, const char **texts,
                                             int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_remove(struct bert_hip_index *ix, int32_t n, const int32_t *ids);
BERT_API int32_t bert_hip_index_n_live(struct bert_hip_index *ix);
BERT_API int32_t bert_hip_index_search_filtered(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t k,
                                                const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_search_filtered_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries,
                                                       int32_t k, const uint32_t *d_allow, int32_t n_words, int32_t *d_ids,
                                                       float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_rescore(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t n_cand,
                                        const int32_t *cand_ids, int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_rescore_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries, int32_t n_cand,
                                               const int32_t *d_cand_ids, int32_t k, int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_search_rescored(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries,
                                                const float *queries, int32_t n_cand, int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_search_rescored_device(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries,
                                                       const float *d_queries, int32_t n_cand, int32_t k, int32_t *d_ids,
                                                       float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_get_rows(struct bert_hip_index *ix, int32_t n, const int32_t *ids, float *rows);
BERT_API int32_t bert_hip_index_partition(struct bert_hip_index *ix, int32_t n_lists, const float *centroids);
BERT_API int32_t bert_hip_index_n_lists(struct bert_hip_index *ix);
BERT_API int32_t bert_hip_index_partition_centroids(struct bert_hip_index *ix, float *centroids);
BERT_API int32_t bert_hip_index_partition_lists(struct bert_hip_index *ix, int32_t *list_of_row);
BERT_API int32_t bert_hip_index_kmeans(struct bert_hip_index *ix, int32_t n_lists, int32_t n_iter, float *centroids);
BERT_API int32_t bert_hip_index_search_probed(struct bert_hip_index *ix, int32_t n_queries, const float *queries, int32_t nprobe,
                                              int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_search_probed_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries,
                                                     int32_t nprobe, int32_t k, int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_search_probed_filtered(struct bert_hip_index *ix, int32_t n_queries, const float *queries,
                                                       int32_t nprobe, int32_t k, const uint32_t *allow, int32_t n_words,
                                                       int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_search_probed_filtered_device(struct bert_hip_index *ix, int32_t n_queries, const float *d_queries,
                                                              int32_t nprobe, int32_t k, const uint32_t *d_allow, int32_t n_words,
                                                              int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_search_rescored_probed(struct bert_hip_index *coarse, struct bert_hip_index *fine, int32_t n_queries,
                                                       const float *queries, int32_t nprobe, int32_t n_cand, int32_t k,
                                                       const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_index_search_rescored_probed_device(struct bert_hip_index *coarse, struct bert_hip_index *fine,
                                                              int32_t n_queries, const float *d_queries, int32_t nprobe,
                                                              int32_t n_cand, int32_t k, const uint32_t *d_allow, int32_t n_words,
                                                              int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_index_partition_save(struct bert_hip_index *ix, const char *path);
BERT_API int32_t bert_hip_index_partition_load(struct bert_hip_index *ix, const char *path);
BERT_API int32_t bert_hip_index_compact(struct bert_hip_index *ix, int32_t *old_ids);
BERT_API int32_t bert_hip_index_save(struct bert_hip_index *ix, const char *path);
BERT_API struct bert_hip_index *bert_hip_index_load(struct bert_ctx *ctx, const char *path);

/* Sparse index: rows of (vocabulary id, weight) terms in HBM on the context's FIRST device (bert_hip_device), exact top-k search by
 * inner product — the consumer of bert_hip_sparse_topk_packed[_device] and bert_hip_encode_sparse_batch.  An index belongs to the
 * context it was made from: bert_free frees any sparse index the caller left alive.  Like every entry point of a context, these
 * functions are not re-entrant on one context.
 *   create   n_vocab: 0 = bert_hip_n_vocab(ctx), else 1 .. 262144.  width: 1 .. 256, the most terms a row can hold.  dtype: 0 = i32
 *            ids + f32 weights (8 bytes per term), 1 = u16 ids + f16 weights (4 bytes per term; the weights rounded to nearest even),
 *            which needs n_vocab <= 65536.  Memory: 64-row blocks of width terms each, plus 4 bytes per row.  NULL + a line on stderr
 *            on error (tokenizer-only context, no device, bad arguments, dtype 1 with a larger vocabulary).
 *   rows and queries   both in the form bert_hip_sparse_topk_packed writes: k_in (rows) or kq (queries) columns per entry, ids [n][k_in]
 *            i32 and weights [n][k_in] f32, in any order; id -1 marks an unused place, whose weight is ignored.  1 <= k_in <= width,
 *            1 <= kq <= 256.  So the MLM head's device output feeds add_device and search_device as it is.
 *   add      appends n rows; they get ids size, size + 1, ...; returns the first new id, negative on error (index unchanged).
 *            add_device: the rows in device memory of the index's device, enqueued on `stream`.  add_texts: runs the MLM head's
 *            width largest terms of each text (bert_hip_encode_sparse_batch's tokenizing and packing) into a device buffer and adds
 *            from there: the rows never reach the host.  Needs a model with the head and n_vocab equal to the model's, else -2.
 *   search   ids[n_queries][k] and scores[n_queries][k], best first; 0 on success, negative on error (outputs untouched).
 *            search_device: queries and results in device memory, enqueued on `stream`.  search_texts: the queries are texts, their kq
 *            largest terms computed like add_texts's rows and searched from the device buffer.
 *   get_rows the stored rows row_ids[n] (each in [0, size), else -2) as out_ids / out_weights [n][width]: the row's ids ascending,
 *            then -1 with weight +0; an f16 weight comes back exactly converted.  Blocking.
 *   reserve  sizes the storage for n_rows rows and the search workspace for up to n_queries queries with any k' <= k and any kq now,
 *            so that the *_device calls within those bounds never allocate (allocation synchronises the device: illegal under stream
 *            capture).  Without it storage and workspace grow on demand.
 * Checks:
 *   - the host forms (add, search) refuse with -2 after a line on stderr, the index unchanged: an id < -1 or >= n_vocab, an id that
 *     appears twice in one row or query, a weight that is not finite (rows of dtype 1: after rounding to f16).
 *   - the device forms do not look: an id outside [0, n_vocab) counts as -1; a repeated id or a non-finite weight leaves that row's or
 *     that query's scores unspecified; nothing is read or written out of bounds in either case.
 *   - what is stored: negative weights are legal; a weight of 0 is stored as a term; a row may have no terms.
 * Semantics:
 *   - score, all arithmetic f32:  acc = +0; for each stored term (id, w) of the row in ascending id: acc = fmaf(w, q[id], acc), where
 *     q[id] is the query's weight for that id, or +0 where the query does not have it.  For finite operands the result has the same
 *     bits whether the absent terms are skipped or multiplied by zero (the kernel skips them; the one exception is an accumulator that
 *     has underflowed to -0, which a skipped term leaves as it is).  A stored f16 weight enters as its exact f32 value; the queries are
 *     never rounded.
 *   - a row without a matching term scores +0 and competes like any other row (with a query of only -1s every row scores +0 and the
 *     smallest ids win): the caller cuts at score <= 0 if it wants only matches.
 *   - order: larger score first; equal scores (==, so +0 equals -0) smaller id first.  Rows with a NaN score are never returned.
 *     Slots beyond the rows are id -1, score -INFINITY.  An empty index is valid.
 *   - 1 <= k <= 256, anything else is an error; n_queries == 0 is a successful no-op; large n_queries run in internal chunks.
 *   - a row's score for a query depends on that query and that row alone: it has the same bits whatever the other queries of the call,
 *     the number of add calls that built the index, reserved or grown storage, k (top-10 is the first 10 entries of top-100), the
 *     slicing of the rows, and host or device entry point.
 *   - *_device calls are asynchronous on the caller's stream; an index has ONE event, so its eagerly enqueued operations never
 *     overlap, whatever streams they were enqueued on.  Within reserve's bounds they never allocate and are legal under stream
 *     capture: STREAM CAPTURE AND GRAPHS above.
 * Results: -1 without an index (or, for the text forms, a context without a device); -2 after a line on stderr for an argument the
 * entry refuses (the checks above, k_in > width, k or kq out of range, a missing pointer, a model without the head); -3 on a device
 * error; -4 for an exception.  Outputs are untouched on error.
 * Not covered: several GPUs; rows wider than 256 terms.  (A search over an embedding index and a sparse index together: "Hybrid
 * search" below; a term-major image of the rows and a search over it: "Sparse index: postings and the inverted search" below.)    */
struct bert_hip_sparse_index;
BERT_API struct bert_hip_sparse_index *bert_hip_sparse_index_create(struct bert_ctx *ctx, int32_t n_vocab, int32_t width, int32_t dtype);
BERT_API void    bert_hip_sparse_index_free(struct bert_hip_sparse_index *ix);
BERT_API int32_t bert_hip_sparse_index_size(struct bert_hip_sparse_index *ix);
BERT_API int32_t bert_hip_sparse_index_reserve(struct bert_hip_sparse_index *ix, int32_t n_rows, int32_t n_queries, int32_t k);
BERT_API int32_t bert_hip_sparse_index_add(struct bert_hip_sparse_index *ix, int32_t n, int32_t k_in, const int32_t *ids, const float *weights);
BERT_API int32_t bert_hip_sparse_index_add_device(struct bert_hip_sparse_index *ix, int32_t n, int32_t k_in, const int32_t *d_ids,
                                                  const float *d_weights, void *stream);
BERT_API int32_t bert_hip_sparse_index_add_texts(struct bert_hip_sparse_index *ix, int32_t n_threads, int32_t n, const char **texts);
BERT_API int32_t bert_hip_sparse_index_search(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids,
                                              const float *q_weights, int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_sparse_index_search_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *d_q_ids,
                                                     const float *d_q_weights, int32_t k, int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_sparse_index_search_texts(struct bert_hip_sparse_index *ix, int32_t n_threads, int32_t n_queries, const char **texts,
                                                    int32_t kq, int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_sparse_index_get_rows(struct bert_hip_sparse_index *ix, int32_t n, const int32_t *row_ids, int32_t *out_ids,
                                                float *out_weights);

/* Sparse index: removing rows, filtered search, rescoring, compaction, files — worded after the embedding index's ("Removing rows,
 * filtered search, compaction, files" and "Rescoring" above); the error codes are the sparse index's (-1 / -2 / -3 / -4, outputs
 * untouched on error).
 *   remove   marks the rows ids[n] removed and returns how many were newly removed.  A removed row is never returned by search,
 *            search_device, search_texts, the filtered forms or rescore.  Ids are stable and size still counts removed rows; n_live is
 *            size less the removed rows; get_rows still returns a removed row.  An id outside [0, size): -2, the index unchanged.
 *            Repeats and already-removed ids are ignored.  Rows added later are live.  Blocking.
 *   search_filtered[_device]   allow: words [n_words] (device memory for _device), bit b of word w set = row 32 w + b may be returned.
 *            allow == NULL is the plain search and n_words is ignored; n_words < ceil(size / 32): -2.  Words at and beyond
 *            ceil(size / 32) are never read, bits at and beyond size are ignored.  Over the rows that are live AND allowed every promise
 *            of the search holds: the score bits of the unfiltered search, the order rule, -1 / -INFINITY slots when fewer than k
 *            qualify, independence from the other queries, k, the slicing, the add history and host or device entry.  The host form
 *            copies ceil(size / 32) words; the device form reads the caller's words when the search runs.
 *   rescore[_device]   per query q its n_cand candidate rows cand_ids[q][0 .. n_cand) scored with the search's bits, the best k of them
 *            to ids / scores [n_queries][k] in the search's order: for distinct ids, the ids and score bits of search_filtered with that
 *            one query and an allow-list of exactly its candidates.  -1 entries and removed rows are skipped; a repeated id counts as
 *            often as it appears.  1 <= n_cand <= 1024, 1 <= k <= 256 (k may exceed n_cand: -1 / -INFINITY slots).  The host form
 *            checks the queries as search does and refuses an id < -1 or >= size (-2); the device form treats such an id as -1.  The
 *            workspace [n_queries][n_cand] grows on demand and is not part of reserve: call once at the largest shape before a capture.
 *            Hybrid search from public calls: bert_hip_index_search_device writes d_ids [n_queries][k] on a stream; pass them as
 *            d_cand_ids of bert_hip_sparse_index_rescore_device on the same stream (and the reverse through bert_hip_index_rescore_device):
 *            the ids never leave the device.  That ranks one side's top-k by the other side; the exact top-k of a weighted sum of
 *            both scores over all rows is bert_hip_hybrid_search ("Hybrid search" below).
 *   compact  drops the removed rows: the live rows keep their order and stored bits and get ids 0 .. n_live - 1; old_ids (may be NULL)
 *            [n_live] receives their former ids.  Returns the new size.  On an index without removals a no-op that returns size (old_ids
 *            the identity).  Afterwards the index keeps no bitmap and launches the unmasked scan again.  Blocking; allocates.
 *   save     writes path + ".tmp" and renames it to path.  load: a new index of the context from a file, NULL + a line on stderr for
 *            any failure.  A loaded index answers every search with the saved one's bits; its n_vocab need not be the context's (the
 *            text routes still refuse a mismatch).
 * File form (little-endian); the file is exactly this long:
 *   header, 64 bytes: magic "BHIPSPX1", u32 version = 1, u32 dtype, u32 n_vocab, u32 width, u32 n_rows, u32 has_live, 32 zero bytes;
 *   ceil(n_rows / 64) blocks of ids exactly as stored, [block][width][64], i32 (dtype 0) or u16 (dtype 1);
 *   the same blocks of weights, f32 or f16;
 *   n_rows i32 counts;
 *   if has_live: ceil(n_rows / 32) u32 live words, the bits at and beyond n_rows zero.
 * save writes zeros for the rows of the last block at and beyond n_rows (what HBM holds there is unspecified), so a file's bytes are a
 * function of the index's rows and removals alone.  load checks, in this order: the header against the file's length, before anything
 * is allocated (version 1, dtype 0 .. 1, n_vocab 1 .. 262144, width 1 .. 256, has_live 0 .. 1, reserved bytes zero); dtype 1 requires
 * n_vocab <= 65536; every count is in [0, width]; no live bit at or beyond n_rows; every id in a column below its row's count is in
 * [0, n_vocab) — which is what keeps the scan's reads in bounds.  Nothing else is checked: weights load as they are, as add_device
 * would have stored them.                                                                                                            */
BERT_API int32_t bert_hip_sparse_index_remove(struct bert_hip_sparse_index *ix, int32_t n, const int32_t *ids);
BERT_API int32_t bert_hip_sparse_index_n_live(struct bert_hip_sparse_index *ix);
BERT_API int32_t bert_hip_sparse_index_search_filtered(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids,
                                                       const float *q_weights, int32_t k, const uint32_t *allow, int32_t n_words,
                                                       int32_t *ids, float *scores);
BERT_API int32_t bert_hip_sparse_index_search_filtered_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq,
                                                              const int32_t *d_q_ids, const float *d_q_weights, int32_t k,
                                                              const uint32_t *d_allow, int32_t n_words, int32_t *d_ids, float *d_scores,
                                                              void *stream);
BERT_API int32_t bert_hip_sparse_index_rescore(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids,
                                               const float *q_weights, int32_t n_cand, const int32_t *cand_ids, int32_t k, int32_t *ids,
                                               float *scores);
BERT_API int32_t bert_hip_sparse_index_rescore_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *d_q_ids,
                                                      const float *d_q_weights, int32_t n_cand, const int32_t *d_cand_ids, int32_t k,
                                                      int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_sparse_index_compact(struct bert_hip_sparse_index *ix, int32_t *old_ids);
BERT_API int32_t bert_hip_sparse_index_save(struct bert_hip_sparse_index *ix, const char *path);
BERT_API struct bert_hip_sparse_index *bert_hip_sparse_index_load(struct bert_ctx *ctx, const char *path);

/* Sparse index: postings and the inverted search.  The search above reads every stored term of every row for every tile of queries.
 * The postings are a second, term-major image of the stored rows, built on the device from the blocks the index already holds; the
 * inverted search reads only the lists of the terms a query has, keeps one f32 accumulator per row on chip, and selects from those.
 *   invert   builds the postings of all size rows and returns that number (0 for an empty index, which is valid).  Rows are cut into
 *            segments of S rows (the tuning key "sparse_index_segment_rows", read here; S = 2048 unless set); per segment a CSR over the
 *            vocabulary — n_vocab + 1 u32 offsets — and per stored term a u16 row number inside the segment and the weight exactly as
 *            stored.  Memory: about that of the rows again (ceil(size / S) * S * width slots of 6 bytes for dtype 0, 4 bytes for
 *            dtype 1) plus ceil(size / S) * (n_vocab + 1) * 4 bytes of offsets, and as many bytes again while invert runs.  Called again
 *            after adds it rebuilds every segment; later searches equal those of a fresh build either way.  It also grows the search
 *            workspace to what the inverted search needs for the n_queries and k last given to reserve, so that reserve + invert (in
 *            either order) make search_inverted_device legal under stream capture within those bounds.  Blocking; allocates.
 *   inverted_rows   the rows the postings cover; 0 without postings; -1 without an index.
 *   search_inverted[_device]   for every query exactly what bert_hip_sparse_index_search_filtered[_device] returns on the same index
 *            with the same arguments: the same ids and the same score bits.  allow == NULL is the plain search.  The score rule is a
 *            chain in ascending term id; the inverted search walks a query's terms in ascending id and applies the same fmaf steps to
 *            each row's accumulator, from +0, in the same order; absent terms are skipped in both forms, so the -0 footnote above
 *            holds unchanged.  Every promise above carries over: a row without a matching term scores +0 and competes; the order rule
 *            (larger score first, == ties by smaller id, NaN never returned, -1 / -INFINITY slots); 1 <= k <= 256 and 1 <= kq <= 256;
 *            removed rows and allow-lists are honoured; a score's bits do not depend on the other queries of the call, on k, on how
 *            the rows are cut into segments and workgroups, on the add history, or on host or device entry; the one-event rule;
 *            within reserved bounds the device form does not allocate and is legal under stream capture.  Checks, chunking of large
 *            n_queries and error codes are search_filtered's: the host form checks its queries, the device form does not look — an id
 *            outside [0, n_vocab) counts as -1, a repeated id in a row or a query leaves only that row's or that query's scores
 *            unspecified, nothing is read or written out of bounds.
 *   search_inverted_texts   bert_hip_sparse_index_search_texts through the inverted search.
 *   stale postings   rows added since the last invert: every inverted search returns -2 after a line on stderr that says to call
 *            invert (as it does before the first invert); inverted_rows still reports the rows covered.  It never answers over a part
 *            of the rows.  remove keeps the postings: removed rows are dropped at selection.  compact drops them (the ids change;
 *            inverted_rows is 0 until the next invert).  A loaded index has no postings: save writes the rows only.
 * (A hybrid search over the postings: bert_hip_dense_sparse_search_inverted, under "Hybrid search" below.)
 * Not covered: a file form of the postings; dynamic pruning (WAND / max-score) — this search is exact and
 * scores every row that holds a queried term; appending to postings on the device or under capture.                                */
BERT_API int32_t bert_hip_sparse_index_invert(struct bert_hip_sparse_index *ix);
BERT_API int32_t bert_hip_sparse_index_inverted_rows(struct bert_hip_sparse_index *ix);
BERT_API int32_t bert_hip_sparse_index_search_inverted(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq, const int32_t *q_ids,
                                                       const float *q_weights, int32_t k, const uint32_t *allow, int32_t n_words,
                                                       int32_t *ids, float *scores);
BERT_API int32_t bert_hip_sparse_index_search_inverted_device(struct bert_hip_sparse_index *ix, int32_t n_queries, int32_t kq,
                                                              const int32_t *d_q_ids, const float *d_q_weights, int32_t k,
                                                              const uint32_t *d_allow, int32_t n_words, int32_t *d_ids, float *d_scores,
                                                              void *stream);
BERT_API int32_t bert_hip_sparse_index_search_inverted_texts(struct bert_hip_sparse_index *ix, int32_t n_threads, int32_t n_queries,
                                                             const char **texts, int32_t kq, int32_t k, int32_t *ids, float *scores);

/* Hybrid search: the exact top-k, over ALL qualifying rows, of a weighted sum of an embedding index's and a sparse index's scores.
 * `dense` is a bert_hip_index of any dtype (0 .. 3), `sparse` a bert_hip_sparse_index of either dtype.  They may belong to different
 * contexts — a bi-encoder and a model with the MLM head — or to the same one; they must live on the same HIP device (bert_hip_device of
 * their contexts) and have equal size, otherwise -2.  They are meant to hold the same texts in the same order: row id r is the same
 * text in both.
 *   Score.  For query q and row r, D is the score bits bert_hip_index_rescore gives the pair on `dense` (the dense search's chain,
 *     whatever the dtype), S the score bits bert_hip_sparse_index_rescore gives it on `sparse` (the fmaf chain from +0; +0 for a row
 *     without a matching term).  The hybrid score is  H = (w_dense * D) + (w_sparse * S):  two f32 multiplications and one f32
 *     addition, each rounded to nearest even, never an fma — NumPy float32 arithmetic reproduces it exactly.  w_dense and w_sparse
 *     must be finite (any sign, zero included), otherwise -2.  NaN and inf follow IEEE through the rule: an i8 row that held an inf
 *     has D = NaN, hence H = NaN, and is never returned.
 *   Qualifying rows.  A row qualifies if it is live in `dense`, live in `sparse` and allowed: allow == NULL means all rows (n_words
 *     is ignored), else words [n_words] as search_filtered's, n_words >= ceil(size / 32) or -2; words at and beyond ceil(size / 32)
 *     are never read, bits at and beyond size are ignored.
 *   Order, slots, limits: the indexes' rules.  A larger H first, equal H (==) by smaller id, NaN never returned, id -1 / score
 *     -INFINITY in the slots beyond the qualifying rows.  1 <= k <= 256, 1 <= kq <= 256.  n_queries == 0 is a successful no-op; an
 *     empty pair of indexes is valid.  queries [n_queries][dim of dense], q_ids / q_weights [n_queries][kq].  The host form checks
 *     its queries as bert_hip_index_search and bert_hip_sparse_index_search check theirs; the device form does not look.
 *   Determinism.  A (query, row) pair's H has the same bits whatever the other queries of the call, k (top-10 is the first 10 of
 *     top-100), the internal chunking of the queries, the number of add calls that built either index, reserved or grown storage, and
 *     host or device entry point.  Hence, with finite D and S, weights (1, 0) return the ids of bert_hip_index_search_filtered and
 *     numerically equal scores (only the sign of a zero may differ), and (0, 1) those of bert_hip_sparse_index_search_filtered.
 *   Streams.  search_device is asynchronous on the caller's stream.  The call is ONE operation of both indexes: it waits for both
 *     indexes' events and leaves both recorded.  Within the bounds of bert_hip_hybrid_reserve — both indexes' reserve for n_rows,
 *     n_queries, k, and the hybrid workspace: at most 256 MiB of dense scores per internal chunk of queries (one query's scores where
 *     those alone are more), and one bitmap — it never allocates and is legal under stream capture (STREAM CAPTURE AND GRAPHS above);
 *     without a reserve everything grows on demand.  The tuning key "hybrid_chunk_queries" (bert_hip_set_option on the SPARSE index's
 *     context) is read when a search is planned and when reserve sizes the workspace: set it before bert_hip_hybrid_reserve.
 *   search_texts.  dense's context encodes the texts as bert_hip_index_search_texts does (dim == n_embd required), sparse's context
 *     runs the MLM head's top-kq as bert_hip_sparse_index_search_texts does and refuses what it refuses (no head, another vocabulary);
 *     the search then runs on the sparse index's stream.  One context may serve both.  A dense context over several GPUs encodes
 *     through bert_hip_encode_batch, as bert_hip_index_search_texts does there; the sparse side uses its context's first device.
 *   Over the postings.  bert_hip_dense_sparse_search_inverted, _inverted_device and _inverted_texts take the arguments of
 *     bert_hip_hybrid_search, _search_device and _search_texts and return, for every query, exactly their ids and score bits on the
 *     same pair of indexes: the same D (the same dense pass), the same S (the inverted search's chain, which is the row-major one:
 *     "postings and the inverted search" above) and the same three rounded operations.  Every rule of this section holds for them
 *     unchanged — score, qualifying rows, order and slots, limits, determinism, the one operation of both indexes, the error codes.
 *     They read the sparse index's postings where the hybrid entries read its rows, and cost less (README, "Hybrid search").  The
 *     postings must cover every row: without them, or with stale ones (rows added since bert_hip_sparse_index_invert, or the index
 *     compacted or loaded), each of the three returns -2 after a line on stderr that says to call bert_hip_sparse_index_invert; it
 *     never answers over a part of the rows.  remove on either index keeps the postings valid.  Within bert_hip_hybrid_reserve and
 *     bert_hip_sparse_index_invert, called in either order, the device form never allocates and is legal under stream capture.
 * Results: 0; -1 without one of the indexes; -2 after a line on stderr for an argument the entry refuses; -3 on a device error; -4 for
 * an exception.  Outputs are untouched on error.
 * Not covered: reciprocal-rank fusion; a probed (IVF) dense side; several GPUs; a hybrid rescore (the two rescores chained give that).   */
BERT_API int32_t bert_hip_hybrid_reserve(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_rows, int32_t n_queries,
                                         int32_t k);
BERT_API int32_t bert_hip_hybrid_search(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries, const float *queries,
                                        int32_t kq, const int32_t *q_ids, const float *q_weights, float w_dense, float w_sparse,
                                        const uint32_t *allow, int32_t n_words, int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_hybrid_search_device(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries,
                                               const float *d_queries, int32_t kq, const int32_t *d_q_ids, const float *d_q_weights,
                                               float w_dense, float w_sparse, const uint32_t *d_allow, int32_t n_words, int32_t k,
                                               int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_hybrid_search_texts(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_threads,
                                              int32_t n_queries, const char **texts, int32_t kq, float w_dense, float w_sparse, int32_t k,
                                              int32_t *ids, float *scores);
BERT_API int32_t bert_hip_dense_sparse_search_inverted(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse, int32_t n_queries,
                                                       const float *queries, int32_t kq, const int32_t *q_ids, const float *q_weights,
                                                       float w_dense, float w_sparse, const uint32_t *allow, int32_t n_words, int32_t k,
                                                       int32_t *ids, float *scores);
BERT_API int32_t bert_hip_dense_sparse_search_inverted_device(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse,
                                                              int32_t n_queries, const float *d_queries, int32_t kq, const int32_t *d_q_ids,
                                                              const float *d_q_weights, float w_dense, float w_sparse,
                                                              const uint32_t *d_allow, int32_t n_words, int32_t k, int32_t *d_ids,
                                                              float *d_scores, void *stream);
BERT_API int32_t bert_hip_dense_sparse_search_inverted_texts(struct bert_hip_index *dense, struct bert_hip_sparse_index *sparse,
                                                             int32_t n_threads, int32_t n_queries, const char **texts, int32_t kq,
                                                             float w_dense, float w_sparse, int32_t k, int32_t *ids, float *scores);

/* TOKEN INDEX: documents' f16 token rows in HBM on the context's FIRST device (bert_hip_device), exact top-k search by late
 * interaction — over ALL stored documents d, the k largest  score(q, d) = sum over the query's tokens i of ( max over the document's
 * tokens j of <Q_i, D_j> )  (ColBERT-style retrieval).  The consumer of bert_hip_eval_packed_tokens[_device] and
 * bert_hip_encode_tokens_batch, and the index form of bert_hip_maxsim[_device] ("token rows and late interaction" above).  An index
 * belongs to the context it was made from: bert_free frees any token index the caller left alive.  Like every entry point of a
 * context, these functions are not re-entrant on one context.
 *   create   dim: 0 = bert_n_embd(ctx), else a multiple of 8 in 8 .. 1024.  Memory: 2 dim bytes per token and 4 bytes per document.
 *            NULL + a line on stderr on error (tokenizer-only context, no device, bad dim).
 *   documents and queries   packed rows [n_tokens][dim] with cumulative lengths cu [n + 1], as bert_hip_encode_tokens_batch writes
 *            them: entry i is rows cu[i] .. cu[i + 1] - 1.  cu ascends strictly from cu[0] >= 0 (every entry has at least one token);
 *            the rows in front of cu[0] are not read.  The total token count of an index stays below 2^31.
 *   add      appends n_docs documents; they get ids size, size + 1, ...; returns the first new id, negative on error.  Everything is
 *            validated first: -2 leaves the index unchanged.  add: cu and f32 rows in host memory, uploaded and rounded to f16 (nearest
 *            even) on the device.  add_device: cu in HOST memory, d_rows f16 in device memory (16-byte aligned), indexed by cu, copied
 *            on `stream`.  add_texts: below.  The add forms take host lengths and may grow storage: they are NOT for stream capture.
 *   get_doc  returns document id's length in tokens; iff cap_tokens >= it, rows [length][dim] receives the stored f16 values converted
 *            exactly.  An id outside [0, size): -2.  Blocking.
 *   search   ids [n_queries][k] and scores [n_queries][k], best first; 0 on success, negative on error (outputs untouched).  search:
 *            qcu and f32 rows in host memory (rounded to f16 on the device), blocking.  search_device: d_qcu, d_q (f16, 16-byte aligned)
 *            and the results in device memory, asynchronous on `stream`.
 *   rescore  per query q its n_cand candidates cand_ids[q][0 .. n_cand) scored with the search's bits, the best k of them in the
 *            search's order.  1 <= n_cand <= 1024; an id of -1 is skipped; a repeated id counts as that many candidates; k may exceed
 *            n_cand (-1 / -INFINITY slots).  The host form refuses any id below -1 or at or beyond size (-2); the device form treats
 *            it as no candidate.  d_cand_ids is exactly what bert_hip_index_search_device writes: pass a dense search's d_ids on the
 *            same stream and its candidates are rescored without leaving the device.  A query may have any length here (no LDS limit:
 *            rescore runs bert_hip_maxsim_device's kernel on the index's rows).  The workspace [n_queries][n_cand] grows on demand
 *            and is not part of reserve: call once at the largest shape before a capture.
 *   reserve  sizes the storage for n_docs documents of n_tokens tokens in all and the search workspace for up to n_queries queries of up
 *            to max_q_len tokens with any k' <= k now, so that search_device within those bounds never allocates.
 *   max_query_tokens   the longest query a SEARCH accepts at this dim (below).
 * Semantics:
 *   - Score.  score(q, d) is the value bert_hip_maxsim_device gives the pair in mode 0 (sum) on the same f16 rows: every inner product
 *     is the f16 chain of the embedding index (f32 accumulation, k ascending, the document block as the A operand); the max is exact;
 *     the query tokens go in blocks of 32, a block's 32 maxima are added in the fixed butterfly order of a wavefront sum with +0 in the
 *     unused lanes, and the blocks' sums are added in ascending order from +0.  Equality is == on floats; for every non-zero score it is
 *     equality of bits; the sign of a zero is not promised.  Masking is maxsim's: a document slot behind the document's end enters
 *     the max as -inf, a query slot behind the query's end adds +0, rows outside the pair's two ranges are never read.
 *   - Order and slots: the indexes' rules.  Larger score first, equal scores (==) smaller id first; a NaN score is never returned; slots
 *     beyond the documents that can be returned are id -1 / score -INFINITY.  1 <= k <= 256; n_queries == 0 is a successful no-op; an
 *     empty index is valid; large n_queries run in internal chunks.
 *   - Determinism.  A (query, document) score and a query's result do not depend on the other queries of the call, the number of add
 *     calls that built the index, reserved or grown storage, how the scan is cut into workgroups (the tuning key "token_index_slices"),
 *     k (top-10 is the first 10 of top-100), the host or device entry point, or search against rescore.
 *   - Query length of a search.  The scan stages the whole query in LDS, ceil(n / 32) blocks of 32 (dim + 8) halfs; max_query_tokens
 *     is the largest multiple of 32, at most 128, whose blocks fit the LDS the kernel allows itself: 128 up to dim 384, 96 up to 768,
 *     64 up to 1024.  The host forms refuse a longer query (-2).  max_q_len of search_device (1 .. max_query_tokens) is a promise that
 *     sizes the launch's LDS, as bert_hip_eval_packed_device's max_len is one: a query that is longer than max_q_len, or empty, or
 *     whose d_qcu entries descend or start below 0, gets k slots of -1 / -INFINITY, its neighbours untouched.
 *   - Texts.  add_texts and search_texts tokenize as bert_encode_batch does, with the same truncation, and run the token-rows pass
 *     with flags 1 | 2 (each row over its L2 norm, f16) in chunks of BERT_HIP_CHUNK_TOKENS: add_texts writes straight into the index's
 *     storage, search_texts a device buffer the scan reads in place.  The stored bits are those of bert_hip_encode_tokens_batch
 *     (flags = 1) rounded to f16.  dim must equal n_embd (-2 otherwise); a query text of more than max_query_tokens tokens: -2.
 *   - Streams.  search_device and rescore_device are asynchronous on the caller's stream; an index has ONE event, so its eagerly
 *     enqueued operations never overlap, whatever streams they were enqueued on.  Within the bounds of reserve (and, for rescore, where
 *     a call of the same shape has run before) they allocate nothing and may be captured into a graph: STREAM CAPTURE AND GRAPHS above.
 * Results: -1 without an index; -2 after a line on stderr for an argument the entry refuses; -3 on a device error; -4 for an exception.
 * Outputs are untouched on error.
 * Removing documents, allow-lists, compaction and files: "LATE INDEX" below.
 * Quantised token rows: "TOKEN INDEX, int8 form" below.
 * Not covered: several GPUs; several queries per workgroup sharing document loads; residual token rows; a mean mode.   */
struct bert_hip_token_index;
BERT_API struct bert_hip_token_index *bert_hip_token_index_create(struct bert_ctx *ctx, int32_t dim);
BERT_API void    bert_hip_token_index_free(struct bert_hip_token_index *ix);
BERT_API int32_t bert_hip_token_index_size(struct bert_hip_token_index *ix);
BERT_API int64_t bert_hip_token_index_n_tokens(struct bert_hip_token_index *ix);
BERT_API int32_t bert_hip_token_index_max_query_tokens(struct bert_hip_token_index *ix);
BERT_API int32_t bert_hip_token_index_reserve(struct bert_hip_token_index *ix, int32_t n_docs, int64_t n_tokens, int32_t n_queries,
                                              int32_t max_q_len, int32_t k);
BERT_API int32_t bert_hip_token_index_add(struct bert_hip_token_index *ix, int32_t n_docs, const int32_t *cu, const float *rows);
BERT_API int32_t bert_hip_token_index_add_device(struct bert_hip_token_index *ix, int32_t n_docs, const int32_t *cu, const void *d_rows,
                                                 void *stream);
BERT_API int32_t bert_hip_token_index_add_texts(struct bert_hip_token_index *ix, int32_t n_threads, int32_t n, const char **texts);
BERT_API int32_t bert_hip_token_index_get_doc(struct bert_hip_token_index *ix, int32_t id, float *rows, int32_t cap_tokens);
BERT_API int32_t bert_hip_token_index_search(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *qcu, const float *q_rows,
                                             int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_token_index_search_device(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *d_qcu, const void *d_q,
                                                    int32_t max_q_len, int32_t k, int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_token_index_search_texts(struct bert_hip_token_index *ix, int32_t n_threads, int32_t n_queries, const char **texts,
                                                   int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_token_index_rescore(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *qcu, const float *q_rows,
                                              int32_t n_cand, const int32_t *cand_ids, int32_t k, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_token_index_rescore_device(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *d_qcu, const void *d_q,
                                                     int32_t n_cand, const int32_t *d_cand_ids, int32_t k, int32_t *d_ids, float *d_scores,
                                                     void *stream);

/* LATE INDEX: the token index's life cycle — removing documents, filtered search, compaction, files — worded after the sparse index's
 * ("Sparse index: removing rows, filtered search, rescoring, compaction, files" above).  These functions take the same
 * struct bert_hip_token_index; they are named bert_hip_late_index_* ("late" as in late interaction, as bert-search --late) because the
 * set of exported names that contain token_index is closed.  The error codes are the token index's (-1 / -2 / -3 / -4, outputs
 * untouched on error).
 *   remove   marks the documents ids[n] removed and returns how many were newly removed.  A removed document is never returned by
 *            search, search_device, search_texts, the filtered forms or rescore[_device]: in rescore a removed id is no candidate,
 *            exactly as -1 is.  Ids are stable; size and n_tokens still count removed documents; n_live and n_live_tokens are those
 *            less the removed documents and their rows; get_doc still returns a removed document.  An id outside [0, size): -2, the
 *            index unchanged.  Repeats and already-removed ids are ignored.  Documents added later are live.  Blocking.  The first
 *            remove allocates a bitmap of the document capacity (one bit per document, with a host mirror); afterwards an add within
 *            reserve's bounds still never allocates.
 *   search_filtered[_device]   allow: words [n_words] (device memory for _device), bit b of word w set = document 32 w + b may be
 *            returned.  allow == NULL is the plain search and n_words is ignored; n_words < ceil(size / 32): -2.  Words at and beyond
 *            ceil(size / 32) are never read, bits at and beyond size are ignored.  Over the documents that are live AND allowed every
 *            promise of the TOKEN INDEX block holds: the score bits of the unfiltered search (bert_hip_maxsim_device's), the order
 *            rule, -1 / -INFINITY slots when fewer than k qualify, independence from the other queries, k, the slicing, the add
 *            history and host or device entry.  A document that does not qualify is skipped before any of its rows is read.  The host
 *            form copies ceil(size / 32) words; the device form reads the caller's words when the search runs, allocates nothing
 *            within reserve's bounds and is legal under stream capture.
 *   compact  drops the removed documents: the live ones keep their order and stored bits and get ids 0 .. n_live - 1; old_ids (may be
 *            NULL) [n_live] receives their former ids.  Returns the new size; n_tokens becomes n_live_tokens and the cumulative
 *            lengths are rebuilt.  On an index without removals a no-op that returns size (old_ids the identity).  Afterwards the index
 *            keeps no bitmap and launches the unmasked scan again.  An index whose documents were all removed compacts to a valid
 *            empty index.  Blocking.  It allocates FRESH storage for the live rows and gathers them on the device, so the peak is old
 *            + new; on an allocation failure -3 and the index unchanged.
 *   save     writes path + ".tmp" and renames it to path.  load: a new index of the context from a file, NULL + a line on stderr for
 *            any failure.  A loaded index answers every search and rescore with the saved one's ids and bits; its dim need not be the
 *            context's n_embd (the text routes still refuse a mismatch).  A save with removals keeps the removed documents' rows and
 *            the bitmap: compact first to drop them.  Rows move between the file and HBM in pieces of 32 MiB: no host copy of the
 *            whole index is ever held.
 *   Stream capture.  The bitmap's words are updated in place, so a graph captured while the bitmap exists sees later removes.  The
 *            first remove (unmasked -> masked kernel, a new pointer), a compact and a growth of the storage change the kernel or the
 *            pointers a captured search holds: capture the graph again after any of them.
 * File form (little-endian); the file is exactly this long:
 *   header, 64 bytes: magic "BHIPTOK1", u32 version = 1, u32 dim, u32 n_docs, u32 has_live, u64 n_tokens, 32 zero bytes;
 *   n_docs + 1 i32 cumulative lengths, starting at 0;
 *   n_tokens x dim f16 rows exactly as stored;
 *   if has_live: ceil(n_docs / 32) u32 live words, the bits at and beyond n_docs zero.
 * A file's bytes are a function of the documents and removals alone.  load checks, in this order: the header against the file's
 * length, before anything is allocated (version 1, dim a multiple of 8 in 8 .. 1024, n_tokens < 2^31, n_docs <= n_tokens, has_live
 * 0 .. 1, reserved bytes zero; the length in 64-bit arithmetic: the largest file needs 42 bits); the cumulative lengths start at 0,
 * ascend strictly and end at n_tokens — which is what keeps the scan's reads in bounds; no live bit at or beyond n_docs.  Rows load as
 * they are.                                                                                                                          */
BERT_API int32_t bert_hip_late_index_remove(struct bert_hip_token_index *ix, int32_t n, const int32_t *ids);
BERT_API int32_t bert_hip_late_index_n_live(struct bert_hip_token_index *ix);
BERT_API int64_t bert_hip_late_index_n_live_tokens(struct bert_hip_token_index *ix);
BERT_API int32_t bert_hip_late_index_search_filtered(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *qcu, const float *q_rows,
                                                     int32_t k, const uint32_t *allow, int32_t n_words, int32_t *ids, float *scores);
BERT_API int32_t bert_hip_late_index_search_filtered_device(struct bert_hip_token_index *ix, int32_t n_queries, const int32_t *d_qcu,
                                                            const void *d_q, int32_t max_q_len, int32_t k, const uint32_t *d_allow,
                                                            int32_t n_words, int32_t *d_ids, float *d_scores, void *stream);
BERT_API int32_t bert_hip_late_index_compact(struct bert_hip_token_index *ix, int32_t *old_ids);
BERT_API int32_t bert_hip_late_index_save(struct bert_hip_token_index *ix, const char *path);
BERT_API struct bert_hip_token_index *bert_hip_late_index_load(struct bert_ctx *ctx, const char *path);

/* TOKEN INDEX, int8 form: the same index with every token row stored as int8 codes and one f32 scale — dpad + 4 bytes per token (dpad:
 * dim rounded up to a multiple of 32) against 2 dim: 388 against 768 at dim 384, 132 against 256 at dim 128, a ratio of
 * (dpad + 4) / (2 dim).  The struct and every entry point of the two blocks above are shared: add (f32 host rows), add_device (f16 device
 * rows), add_texts, get_doc, search, search_device, search_texts, rescore, rescore_device, reserve, size, n_tokens, max_query_tokens,
 * remove, n_live, n_live_tokens and search_filtered[_device] take an int8 index with the inputs they take today.  The new names are
 * bert_hip_late_index_* for the reason given under LATE INDEX.
 *   create   dtype 1: the f16 form — exactly bert_hip_token_index_create(ctx, dim) —; dtype 2: the int8 form (the embedding index's code
 *            for it); anything else: NULL + a line on stderr.  dim as there.
 *   dtype    1 or 2; -1 without an index.
 *   get_codes   returns document id's length in tokens; iff cap_tokens >= it (and both pointers are given), codes [length][dpad] and
 *            scales [length] receive the stored form.  An f16 index, or an id outside [0, size): -2.  Blocking.
 * Semantics:
 *   - Stored rows.  The embedding index's int8 rule, per token: scale = amax / 127 in f32; code_i = clamp(rint(x_i / scale), -127, 127)
 *     with IEEE division and round to nearest even; every code 0 where the scale is 0; where an element is NaN or +-inf the scale is
 *     NaN and the codes are 0.  The padding up to dpad is zero.  f16 rows (add_device, the text routes) are converted to f32 exactly
 *     and follow the same rule; add quantises its f32 rows as they are, without a detour through f16.  get_doc returns
 *     (float)code * scale.
 *   - Queries are quantised the same way, per token, on the device, into a workspace that reserve sizes with the search's: a
 *     search_device within reserve's bounds still allocates nothing and may be captured.  The host forms quantise the f32 rows as
 *     they are; the device forms and search_texts the f16 rows.
 *   - Score.  With dot_ij = sum over e of qc_i[e] dc_j[e], an exact int32:  m_i = max over j of ((float)dot_ij * ds_j)  (the
 *     conversion is exact, |dot| <= 1024 x 127^2 < 2^24; a document slot behind the document's end enters as -inf);  t_i = m_i * qs_i,
 *     one multiply per query token behind the max;  the t_i are added exactly as the f16 form adds its maxima — blocks of 32 in the
 *     butterfly order of a wavefront sum with +0 in the unused lanes and behind the query's end, the blocks' sums in ascending order
 *     from +0.  Every operation is exact or one correctly rounded f32 operation in this order, so the score's bits are a function of
 *     the two sets of rows alone, and the determinism, order and slot rules of the TOKEN INDEX block hold word for word (slicing, k,
 *     batch neighbours, add history, growth, host or device entry on the same values, search against rescore).
 *   - Non-finite rows.  A document that holds a token whose scale is NaN scores NaN and is never returned; a query that holds such a
 *     token gets k slots of -1 / -INFINITY, its neighbours untouched.
 *   - Query length.  The query's codes are staged in LDS as rows of dpad + 16 bytes, 512 bytes of scales beside them: 128 tokens fit at
 *     every dim (dim 1024: 137 744 bytes with the longest list), so max_query_tokens is 128 for every int8 index.
 *   - rescore runs the search's kernel over the candidate lists (a workgroup per query and slice of its list, a wave per document as
 *     in the search), not bert_hip_maxsim_device's.  It therefore stages the query as a search does: the host form refuses a query of
 *     more than max_query_tokens tokens (-2), the device form gives it -1 / -INFINITY — where the f16 form's rescore has no limit.
 *     The workspace grows on demand and is not part of reserve, as there.
 * Not covered: compact and save of an int8 index (-2 after a line on stderr, the index unchanged and still searchable), and a file
 * form: bert_hip_late_index_load keeps refusing anything but a BHIPTOK1 version 1 file, which holds f16 rows.                       */
BERT_API struct bert_hip_token_index *bert_hip_late_index_create(struct bert_ctx *ctx, int32_t dim, int32_t dtype);
BERT_API int32_t bert_hip_late_index_dtype(struct bert_hip_token_index *ix);
BERT_API int32_t bert_hip_late_index_get_codes(struct bert_hip_token_index *ix, int32_t id, int8_t *codes, float *scales, int32_t cap_tokens);

BERT_API const char *bert_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* BERT_HIP_H */
