/* bert_hip_test.h — op-level test hooks of the MI355X engine: standalone kernel entry points (host buffers in, host
 * buffers out) that the parity tests call through ctypes.  They live in libbert_test.so (libbert.so plus these), NOT in
 * the product library.
 */
#ifndef BERT_HIP_TEST_H
#define BERT_HIP_TEST_H

#include "bert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The batch-route kernels compute whole tiles of 128 or 256 tokens, and in the engine's grow-only workspaces the rows behind a
 * call's last token (and every row a pass has not written yet) hold what an earlier pass left.  The entries below allocate per
 * call; this process-wide setting is what they put where the engine would have stale data, BEFORE the first launch:
 *   - rows M .. M_pad - 1 of every token-row input (A, resid, r and its row statistics, ctx, x; attention: the rows of qkv and of x
 *     behind the last sentence, to the end of its tile and one tile of 128 more, which no kernel may read) hold pattern16
 *     (pattern32 in 32-bit buffers);
 *   - every output and intermediate buffer (C, u, out2, the partial statistics and finalized rows of the LayerNorm fold, qkv
 *     between projection and attention, y and the intermediate of the five-kernel tail, every out) holds it in ALL its words.
 * Entries: bert_hip_test_gemm, _gemm_lnfold, _attention, _qkv_attention, _layer_tail, _embed_ln, _layernorm and the five _f32_ entries (the latency route's
 * entries take a `pad` argument of their own).  0, 0 (the state at load): zeros, as before.  Quiet NaNs (0x7E00, 0x7FC00000) make any read of such a word
 * show in the rows a call returns; to the kernels they are data.  Set it under try / finally: it outlives the call.          */
BERT_API void bert_hip_test_set_pad(uint32_t pattern16, uint32_t pattern32);

/* Standalone kernel entry points for op-level tests (host buffers in, host buffers out).
 * C[M][N] = epilogue(A[M][K] (f16 bits) x W[N][K]^T + bias); W given in file layout of `wtype`
 * (row-major f32 / f16 / block_q4_0 / block_q4_1 bytes).  epilogue: 0 bias, 1 bias+GELU(tanh),
 * 2 bias+residual.  impl: 0 tiled MFMA kernel (gemm.hip; q4 blocks dequantised in the tile load), 1 naive, 3 the 256 x 256 tile
 * kernel (gemm256.hip; -2 unless f16/f32 weights and N % 256 == 0).  Output f16 bits.  Returns 0 on success.                  */
BERT_API int32_t bert_hip_test_gemm(int32_t M, int32_t N, int32_t K, const uint16_t *A, const void *W,
                                    int32_t wtype, const float *bias, const uint16_t *resid,
                                    int32_t epilogue, int32_t impl, uint16_t *C);

/* LayerNorm folded into the mat-muls around it (kernels.h GemmLnFold; gemm256.hip, f16 weights, H and N2 multiples of 256, M is
 * padded to 256): the pair a layer runs —
 *   u   = A1[M][K1] W1[H][K1]^T + b1 + R,   R = r[M][H] itself (rg == NULL) or LayerNorm(r; rg, rb) rebuilt per element from r's row
 *         statistics (computed here on the host), written UN-normalised with per-row partial statistics;
 *   out = epi2( LayerNorm(u; g, be) W2[N2][H]^T + b2 ),  epi2 0 = bias, 1 = bias + GELU: reads u itself, gamma folded into W2, one
 *         statistics k-step, rows scaled by 1 / std.
 * u_out [M][H], out2 [M][N2] f16 bits, rows_out [M][4] f32 {rstd, -mean rstd, -mean, std} of u.  Returns 0 on success, -3 when
 * gemm256 has no kernel for the folded form asked for (any other epi2: the second mat-mul is not launched).                      */
BERT_API int32_t bert_hip_test_gemm_lnfold(int32_t M, int32_t K1, int32_t H, int32_t N2, const uint16_t *A1, const uint16_t *W1,
                                           const float *b1, const uint16_t *r, const float *rg, const float *rb,
                                           const uint16_t *W2, const float *b2, const float *g, const float *be, int32_t epi2,
                                           uint16_t *u_out, uint16_t *out2, float *rows_out);

/* qkv[T][3H] f16 bits (Q | K | V per row), packed sentences -> ctx[T][H] f16 bits.             */
BERT_API int32_t bert_hip_test_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head,
                                         int32_t d_head, const uint16_t *qkv, int32_t impl, uint16_t *out);
/* The same with MPNet's relative position bias: W [32][n_head] f32 (HuggingFace's encoder.relative_attention_bias.weight), expanded for
 * sentences of up to P tokens as the engine expands it at load (bert_hip_test_rel_bias_table; times sqrt(d_head) for impl 0, whose kernel
 * scales the sum).  impl 0 = the matrix-core kernel, 1 = the naive one.  rel, if not NULL, is a table [n_head][2 P - 1] f32 taken AS IT
 * IS in place of W's expansion (W may then be NULL): what a test poisons outside a sentence's window.  -1 for a sentence longer than P. */
BERT_API int32_t bert_hip_test_attention_bias(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head,
                                              const uint16_t *qkv, int32_t impl, uint16_t *out, const float *W, int32_t P, const float *rel);
/* The host expansion alone (weights.h rel_bias_table, no device): out [n_head][2 P - 1], out[h][d + P - 1] = W[bucket(d)][h].  0, or -1
 * for a NULL pointer, n_head < 1 or P < 1.                                                                                          */
BERT_API int32_t bert_hip_test_rel_bias_table(const float *W, int32_t n_head, int32_t P, float *out);

/* Q|K|V projection + attention: x[T][H] f16 bits, Wqkv [3H][H] (Q rows, K rows, V rows) in file layout of `wtype`,
 * bias[3H] -> ctx[T][H] f16 bits (reference bert.cpp:822-856).  fused: 0 = GEMM kernel + attention kernel; the window kernel
 * (qkv_attention2.hip; -2 if the shape is not supported) with 2 = next-fit windows built on the host, 3 = the uniform
 * placement rule, 4 = next-fit windows built on the device; 5 = the first half of a latency-route layer: the feature-split
 * projection kernel (skinny.hip, x as f16 rows) + the attention kernel (-2 unless the latency route takes the shape).       */
BERT_API int32_t bert_hip_test_qkv_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head,
                                             int32_t d_head, const uint16_t *x, const void *Wqkv, int32_t wtype,
                                             const float *bias, int32_t fused, uint16_t *out);

/* Everything of a layer after the attention (reference bert.cpp:859-901):
 *   y = LayerNorm(ctx Wo^T + bo + x) * g1 + be1;  out = LayerNorm(gelu(y W1^T + b1) W2^T + b2 + y) * g2 + be2
 * ctx, x, out [M][H] f16 bits; Wo [H][H], W1 [I][H], W2 [H][I] in file layout of `wtype`.
 * impl: 0 = GEMM + LayerNorm kernels, 1 = the one-launch kernel with specialist wave pairs (layer_tail.hip; -2 if the shape is
 * not supported).  q4 `wtype`: both keep the blocks 4-bit on the device and dequantise in the tile load.             */
BERT_API int32_t bert_hip_test_layer_tail(int32_t M, int32_t H, int32_t I, const uint16_t *ctx, const uint16_t *x,
                                          const void *Wo, const void *W1, const void *W2, int32_t wtype,
                                          const float *bo, const float *g1, const float *be1, const float *b1,
                                          const float *b2, const float *g2, const float *be2, int32_t impl,
                                          uint16_t *out);

/* The same layer tail through the kernels of the latency route (skinny.hip), launched as Engine::forward_latency launches them:
 * out-projection, up-projection with LayerNorm 1, down-projection, LayerNorm 2, on ceil(M / 32) token blocks.  Inputs as above
 * (-2 unless skinny_layer_supported takes the matrices).  pad: the 16-bit pattern rows M .. M_pad - 1 of the ctx and x buffers
 * hold (M_pad: M rounded up to 128; the kernels compute whole blocks of 32 tokens and read those rows).  Besides out [M][H],
 * each unless NULL: v_proj f32 [M][H] = ctx Wo^T + bo + x, y f16 [M][H] = LayerNorm 1 of it, ff f16 [M][I] = gelu(y W1^T + b1)
 * in the kernels' fragment order (inside every group of 16 features the runs of 4 sit at [0-3, 8-11, 4-7, 12-15]),
 * v_down f32 [M][H] = ff W2^T + b2 + y.                                                                                      */
BERT_API int32_t bert_hip_test_skinny_tail(int32_t M, int32_t H, int32_t I, const uint16_t *ctx, const uint16_t *x, const void *Wo,
                                           const void *W1, const void *W2, int32_t wtype, const float *bo, const float *g1,
                                           const float *be1, const float *b1, const float *b2, const float *g2, const float *be2,
                                           uint32_t pad, uint16_t *out, float *v_proj, uint16_t *y, uint16_t *ff, float *v_down);

/* The Q|K|V projection of the latency route: qkv [M][3H] f16 bits = rows Wqkv^T + bias, Wqkv [3H][H] in file layout of `wtype`.
 * Exactly one of x and V: the rows are x [M][H] f16 bits (the first layer's form), or LayerNorm(V [M][H] f32; gamma, beta), which
 * the kernel computes itself and also writes to ln_out [M][H] f16 bits (every later layer's form).  pad: what rows M .. M_pad - 1
 * of the x or V buffer hold, a 16-bit resp. 32-bit pattern.  -2 unless the latency route takes the shape.                      */
BERT_API int32_t bert_hip_test_skinny_qkv(int32_t M, int32_t H, const uint16_t *x, const float *V, const float *gamma,
                                          const float *beta, const void *Wqkv, int32_t wtype, const float *bias, uint32_t pad,
                                          uint16_t *qkv, uint16_t *ln_out);

/* The f16 row kernels of misc_kernels.hip, launched as the engine launches them.  Token-row buffers have the engine's workspace shape,
 * whole tiles of 256 rows: under bert_hip_test_set_pad the rows behind the last token hold pattern16 (the embedding's output buffer
 * holds it in ALL its words before the launch), and an entry returns -4 if a word behind the last token's row has changed afterwards.
 * -1: bad arguments or a HIP error.
 * Embedding gather-sum + LayerNorm (reference bert.cpp:796-814): tables in the file layout of `table_type` (0 f32, 1 f16,
 * 2 q4_0, 3 q4_1), word [n_vocab][H], type [2][H] (row 0 is used), pos [n_pos][H]; packed sentences; out [T][H] f16 bits.  Ids outside
 * [0, n_vocab) take row 0 resp. n_vocab - 1.  max_len is the caller's promise as bert_hip_eval_packed_device takes it (0: the longest
 * sentence; <= n_pos, -1 otherwise): it chooses the grid form, and no position row at or behind max_len is read.  Rows of a sentence
 * longer than max_len behind its place round_up(max_len, 4) may keep the pattern.                                                   */
BERT_API int32_t bert_hip_test_embed_ln(int32_t table_type, int32_t H, int32_t n_vocab, int32_t n_pos, const void *word,
                                        const void *type, const void *pos, const float *gamma, const float *beta,
                                        const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences,
                                        int32_t max_len, uint16_t *out);
/* The same arguments and values in LANE ORDER (launch_embed_ln_lanes, the one-launch route's embedding on full windows): out gets the
 * [T][H] f16 bits as stored — 32-token block k at 32 k H, its fragment q at + 512 q, lane l = 32 hi + l31 of it at + 8 l: features
 * 16 q + 4 hi + {0..3}, 16 q + 8 + 4 hi + {0..3} of token 32 k + l31.  Every token in front of T is written.  -2, and nothing is
 * launched, for a shape the launcher declines (T no positive multiple of 128, H not 256 or 384, a table type outside 0..3).          */
BERT_API int32_t bert_hip_test_embed_ln_lanes(int32_t table_type, int32_t H, int32_t n_vocab, int32_t n_pos, const void *word,
                                              const void *type, const void *pos, const float *gamma, const float *beta,
                                              const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences,
                                              int32_t max_len, uint16_t *out);
/* out [T][H] = LayerNorm(x [T][H]) gamma + beta on f16 rows, in place on the device as in the engine (launch_layernorm: two-pass
 * statistics, eps 1e-5); H even, at most 4096.                                                                                      */
BERT_API int32_t bert_hip_test_layernorm(int32_t T, int32_t H, const uint16_t *x, const float *gamma, const float *beta, uint16_t *out);
/* Mean-pool + L2 normalise (reference bert.cpp:904-913) of x [T][H] f16 bits -> out [n_sentences][H] f32; *status receives
 * the device status word (1 if a sentence length is outside [1, max_len]: its row is NaN).                              */
BERT_API int32_t bert_hip_test_pool_normalize(int32_t H, const uint16_t *x, const int32_t *cu_seqlens, int32_t n_sentences,
                                              int32_t max_len, float *out, int32_t *status);
/* The same kernel under the settings of a context (bert_hip.h): pooling 0 mean | 1 the sentence's first row, normalize 1 | 0.   */
BERT_API int32_t bert_hip_test_pool(int32_t H, const uint16_t *x, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len,
                                    int32_t pooling, int32_t normalize, float *out, int32_t *status);

/* Grouped pooling (bert_hip.h "long texts"; launch_group_pool) on chosen rows and weights: rows f32 [n_rows][H]; weights [n_rows] > 0
 * (the sentences' token counts), or NULL: 1 each; group g = rows group_cu[g] .. group_cu[g + 1] - 1 (n_groups + 1 entries; group_cu[0]
 * may lie behind row 0 and the last entry in front of n_rows: the rows around the groups are the caller's to poison); raw 1: the
 * weighted means, 0: divided by their L2 norms.  out [n_groups][H]: uploaded as the caller filled it, so a word the kernel does not
 * write comes back as it was.  *status (nullable) receives the device status word: 1 if a group is empty, not ascending or outside
 * [0, n_rows] (its row is NaN).  -1: bad arguments or a HIP error.                                                                  */
BERT_API int32_t bert_hip_test_group_pool(const float *rows, int32_t n_rows, const int32_t *weights, const int32_t *group_cu,
                                          int32_t n_groups, int32_t H, int32_t raw, float *out, int32_t *status);

/* The f32 route's kernels (f32_route.hip: what an f32 model file runs on), each launched exactly as Engine::forward_f32 launches it;
 * everything f32.  Token-row buffers have the engine's workspace shape, whole tiles of 256 rows: under bert_hip_test_set_pad the rows
 * behind the last token of every input hold pattern32, every output buffer holds it in ALL its words before the launch, and an entry
 * returns -4 if a word behind the last token's row has changed afterwards.  -1: bad arguments or a HIP error.
 * C [M][N] = epilogue(A [M][K] W [N][K]^T + bias [N]), epilogue 0 bias, 1 bias + GELU (tanh), 2 bias + resid [M][N] (else resid NULL).  */
BERT_API int32_t bert_hip_test_f32_gemm(int32_t M, int32_t N, int32_t K, const float *A, const float *W, const float *bias,
                                        const float *resid, int32_t epilogue, float *C);
/* qkv [T][3H] (Q | K | V per row), packed sentences -> out [T][H].  max_len is the caller's: it sizes the grid and each wave's stripe
 * of scores in LDS.  The rows of a sentence longer than max_len are not written (they keep the pattern).  -2, and no launch, when
 * max_len needs more dynamic LDS than the device gives a workgroup.                                                              */
BERT_API int32_t bert_hip_test_f32_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head,
                                             int32_t max_len, const float *qkv, float *out);
/* The same with MPNet's relative position bias, W [32][n_head] f32 expanded for sentences of up to P tokens (P >= max_len, -1 otherwise). */
BERT_API int32_t bert_hip_test_f32_attention_bias(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head,
                                                  int32_t max_len, const float *qkv, float *out, const float *W, int32_t P);
/* out [T][H] = LayerNorm(x [T][H]) gamma + beta, two-pass statistics, eps 1e-5.                                                  */
BERT_API int32_t bert_hip_test_f32_layernorm(int32_t T, int32_t H, const float *x, const float *gamma, const float *beta, float *out);
/* Embedding gather-sum + LayerNorm on f32 tables: word [n_vocab][H], type [2][H] (row 0 is used), pos [n_pos][H]; out [T][H].
 * max_len <= n_pos as bert_hip_eval_packed_device demands (-1 otherwise): no position row at or behind max_len is read.          */
BERT_API int32_t bert_hip_test_f32_embed_ln(int32_t H, int32_t n_vocab, int32_t n_pos, const float *word, const float *type,
                                            const float *pos, const float *gamma, const float *beta, const bert_vocab_id *tokens,
                                            const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len, float *out);
/* bert_hip_test_pool on f32 rows x [T][H]: out [n_sentences][H], *status the device status word.                                  */
BERT_API int32_t bert_hip_test_f32_pool(int32_t H, const float *x, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len,
                                        int32_t pooling, int32_t normalize, float *out, int32_t *status);

/* Parses a model file (no GPU): returns the number of tensors (negative on error, message on stderr), whether the file uses the
 * legacy 20 / 24-byte q4 blocks, and a digest of every tensor's name, type and bytes AFTER conversion to the current layout.   */
BERT_API int32_t bert_hip_test_model_digest(const char *fname, int32_t *legacy_q4, uint64_t *digest);

/* The host side of the weight packing (no GPU): W [N][K] in the file layout of `wtype` (0 f32, 1 f16, 2 q4_0, 3 q4_1) -> the bytes
 * of one image as the engine uploads it (kernels.h GemmWeight / GemmLnFold).  form: 0 the f16 image [N_pad][K] (N_pad: N rounded up
 * to 128, the padding rows zero), 1 the same with k order [0-3, 8-11, 4-7, 12-15] inside every group of 16, 2 the q4 nibble plane,
 * 3 the q4 scale plane (index ((nt (K/64) + kt) 128 + row) 2 + block; q4 `wtype`, K % 64 == 0, N % 8 == 0), 4 the LayerNorm-fold
 * image [N_pad][K] = f16(W diag(gamma)), 5 the fold's statistics columns [N][16] f16 (gamma, beta; bias may be NULL), 6 the packed
 * words [N] f16 gamma | f16 (beta + bias) << 16 (W, wtype and K unused), 7 an embedding table of a q4 file as f32 [N][K].
 * form | BERT_HIP_TEST_PACK_STACK3: W is three tensors of N / 3 rows, one behind the other, packed as one stacked matrix (forms 0-5).
 * Returns the bytes written to `out` (capacity out_cap), -1 for a request that makes no sense, -2 when out_cap is too small.      */
#define BERT_HIP_TEST_PACK_STACK3 0x100
BERT_API int32_t bert_hip_test_pack_weight(const void *W, int32_t wtype, int32_t N, int32_t K, int32_t form, const float *gamma,
                                           const float *beta, const float *bias, void *out, int64_t out_cap);

/* Host logic of the multi-GPU layer and of the sentence windows, callable without a GPU:
 * shard bounds [n_shards + 1] of a packed batch (multi_device.h), and the {first, count} windows of 128 token slots
 * (engine.h build_windows; returns their number, `windows` holds 2 ints per window, capacity n_sentences).        */
BERT_API void bert_hip_test_shard_bounds(const int32_t *cu_seqlens, int32_t n_sentences, int32_t n_shards, int32_t *bounds);
BERT_API int32_t bert_hip_test_build_windows(const int32_t *cu_seqlens, int32_t n_sentences, int32_t *windows);
/* Upper bound of the number of windows used to size the grid of the fused attention kernel when the windows are built on the
 * device (a function of the sentence and token counts only).                                                             */
BERT_API int32_t bert_hip_test_max_windows(int32_t n_sentences, int32_t n_tokens);
/* the windows' place granularity in THIS library (16, or 8: BERT_HIP_WINDOW_SLOTS / option "window_slots"); returns the value now in force */
BERT_API int32_t bert_hip_test_set_window_slots(int32_t slots);
/* The same windows from the device-side builder the asynchronous device API uses (needs a GPU; -1 on a HIP error).        */
BERT_API int32_t bert_hip_test_build_windows_device(const int32_t *cu_seqlens, int32_t n_sentences, int32_t *windows);
/* The multi-device dispatcher (shards, a persistent worker thread per shard beyond the first, results straight into the
 * caller's rows) driven with a stub evaluator instead of GPUs: row b of `out` [n_sentences][H] becomes f(sentence b) =
 * {sum of ids, length, shard, ...}.  H < 0: the stub throws inside every shard (the exception must come back as -9).      */
BERT_API int32_t bert_hip_test_dispatch(const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences,
                                        int32_t n_shards, int32_t H, float *out);
/* Threads this process has created for shard work so far (ShardWorkers): repeated calls must not create threads.          */
BERT_API int64_t bert_hip_test_shard_threads_created(void);


/* Host logic of the API layer, callable without a GPU.
 * The device list of BERT_HIP_DEVICES (context.h parse_device_list) on a box of n_devices devices whose caller's current device
 * is `current`: returns the number of devices written to devs (capacity n_devices), or -1 with the message in err (err_cap bytes). */
BERT_API int32_t bert_hip_test_parse_devices(const char *list, int32_t n_devices, int32_t current, int32_t *devs, char *err,
                                             int32_t err_cap);
/* The super-batch cut of bert_hip_eval_packed_gather (gather.h gather_runs): returns the number of entries written to runs
 * (capacity n_sentences + 1).                                                                                                  */
BERT_API int32_t bert_hip_test_gather_runs(const int32_t *cu_seqlens, int32_t n_sentences, int64_t tokens_per_run, int32_t *runs);
/* The group sizes bert_encode_batch cuts n_inputs texts into (text_batch.h encode_group_size): returns their number, the first
 * `cap` of them in groups.                                                                                                      */
BERT_API int32_t bert_hip_test_encode_groups(int32_t n_inputs, int32_t *groups, int32_t cap);
/* The tokenize + validate + pack step of the text entry points (text_batch.h TokenGroup) on the context's first group; works on
 * a tokenizer-only context.  counts == NULL: tokenizes n texts on n_threads threads and packs them.  counts != NULL: the same,
 * but the pack step runs on these n counts instead of the tokenizer's (how a text that cannot be evaluated is produced: the
 * tokenizer truncates, so no text gives a count outside 1 .. n_max_tokens).  n_tokens [n] receives the counts packed with,
 * cu [n + 1] the prefix sums (n_ok + 1 entries are written), packed the ids back to back.  Returns n_ok, the number of texts in
 * front of the first one that cannot be evaluated, or -1 if packed_cap ids do not hold the result.                             */
BERT_API int32_t bert_hip_test_tokenize_pack(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts,
                                             const int32_t *counts, int32_t *n_tokens, int32_t *cu, bert_vocab_id *packed,
                                             int32_t packed_cap);
/* The check bert_hip_index_load runs on a file's header before it allocates (index_file.h index_header_check; the format is in
 * bert_hip.h): buf holds the first buf_len bytes of a file of file_bytes bytes.  0 and fields = {version, dtype, dim, dpad,
 * n_rows, has_live} for a header this build loads; -1 and the reason in err (err_cap bytes) otherwise.                          */
BERT_API int32_t bert_hip_test_index_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err,
                                            int32_t err_cap);
/* The same for a partition file (index_file.h partition_header_check, in front of bert_hip_index_partition_load): 0 and
 * fields = {version, dim, n_lists, n_part}; -1 and the reason in err otherwise.                                             */
BERT_API int32_t bert_hip_test_partition_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err,
                                                int32_t err_cap);

/* The list tables of a partitioned index (partition.h build_lists; bert_hip.h "cluster partition"): offsets[n_lists + 1] and
 * order[up to n] from list_of[n] by a stable counting sort, entries outside [0, n_lists) in no list.  Returns the number of
 * entries written to order, -1 for bad arguments.  No device.                                                               */
BERT_API int32_t bert_hip_test_build_lists(const int32_t *list_of, int32_t n, int32_t n_lists, int32_t *offsets, int32_t *order);

/* launch_token_rows on its own (kernels.h; bert_hip.h "token rows and late interaction"): x [T][H], f16 bits (is_f32 0) or f32 (1), the
 * final states of a pass; cu_seqlens [n_sentences + 1], max_len and flags as bert_hip_eval_packed_tokens_device takes them; out [T][H],
 * f16 bits with flags bit 1, else f32.  Host buffers in and out.  The device copy of x has its rows rounded up to whole 128-token
 * tiles: the rows behind T, and every word of the output before the launch, hold the patterns of bert_hip_test_set_pad.  0, or -1
 * after a line on stderr.                                                                                                        */
BERT_API int32_t bert_hip_test_token_rows(const void *x, int32_t is_f32, int32_t T, int32_t H, const int32_t *cu_seqlens, int32_t n_sentences,
                                          int32_t max_len, int32_t flags, void *out);

/* The embedding kernels with token types (bert_hip.h "sentence pairs and scores"): the arguments of bert_hip_test_embed_ln, _embed_ln_lanes
 * and _f32_embed_ln, plus first_len [n_sentences] (nullable: the untyped instantiation; any value is legal, type [2][H] has both rows
 * read) and the form: 0 the rows kernel on its (group, sentence) grid, 1 the rows kernel with the bisection, 2 the generic kernel, 3 the
 * lane-order kernel (out as _embed_ln_lanes stores it), 4 the f32 route's (table_type 0 only; out [T][H] f32, else f16 bits).  The
 * padding and the -4 check of those entries apply.  -2, and nothing is launched, for a shape the form does not take.                */
BERT_API int32_t bert_hip_test_embed_ln_typed(int32_t table_type, int32_t H, int32_t n_vocab, int32_t n_pos, const void *word,
                                              const void *type, const void *pos, const float *gamma, const float *beta,
                                              const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len,
                                              const int32_t *first_len, int32_t form, void *out);
/* The classification head on its own (kernels.h launch_cls_head / launch_cls_head_f32): rows [B][H] f32, Wp [H][H] as f16 bits
 * (wp_is_f32 0) or f32 (1), bp [H], Wc [n_labels][H], bc [n_labels], flags bit 0 the sigmoid; form 0 the matrix-core kernel (f16 Wp, H % 8
 * == 0, H <= 1024), 1 the plain one; out [B][n_labels].  The device copy of the rows runs one block of 32 sentences past the last whole
 * one, holding pattern32 of bert_hip_test_set_pad, as every word of the output does before the launch; -4 if a word behind the last
 * sentence's scores has changed.  -2, and no launch, for a shape the form does not take.                                            */
BERT_API int32_t bert_hip_test_cls_head(int32_t B, int32_t H, int32_t n_labels, const float *rows, const void *Wp, int32_t wp_is_f32,
                                        const float *bp, const float *Wc, const float *bc, int32_t flags, int32_t form, float *out);

/* The vocabulary launch of the learned sparse embeddings on its own (kernels.h launch_sparse_vocab + launch_sparse_finish, or
 * launch_sparse_vocab_f32): t [T][H] token rows and e [V][H] vocabulary rows as f16 bits or f32 (*_is_f32), bias [V], cu_seqlens
 * [n_sentences + 1] with T = its last entry; sentences s0 .. s0 + ns - 1 are served: out [ns][V].  form 0: the matrix-core kernel (both
 * f16, H % 8 == 0, H <= 1024), 1: the plain one.  On the device 64 NaN rows stand in front of and behind the token rows and behind row V
 * of the vocabulary image, and the output is pre-filled with negative, NaN and huge bit patterns, one row of pattern32 (bert_hip_test_set_pad)
 * behind it; -4 if a word of that row has changed.  -2, and no launch, for a shape the form does not take.                          */
BERT_API int32_t bert_hip_test_sparse_vocab(int32_t form, int32_t H, int32_t V, const void *t, int32_t t_is_f32, const void *e, int32_t e_is_f32,
                                            const float *bias, const int32_t *cu_seqlens, int32_t n_sentences, int32_t s0, int32_t ns, float *out);
/* The top-k launch on its own (kernels.h launch_sparse_topk): w [n][V] -> ids [n][k], weights [n][k]; both outputs hold pattern32 before
 * the launch, one row behind the last included (-4 if that changed).  -2, and no launch, for k outside 1 .. 256 or V >= 2^24.        */
BERT_API int32_t bert_hip_test_sparse_topk(const float *w, int32_t n, int32_t V, int32_t k, int32_t *ids, float *weights);

/* The launch geometry of the kernels whose loops depend on the size of the launch, so that a test can assert the path it reached.
 * The grid the matrix-core vocabulary launch takes for n_embd H, V vocabulary entries, T packed tokens of which ns sentences of at most
 * max_len tokens are served (kernels.h sparse_vocab_geometry; no GPU): geometry = {tile, n_tiles, slab_blocks, n_slabs} — token slots per
 * workgroup, token tiles (grid.x), 32-entry vocabulary blocks per slab (a workgroup's four waves take 8 of them per round, a pair each), slabs
 * (grid.y).  0; -2 and zeros where the launcher refuses the shape; -1 for a NULL geometry.                                          */
BERT_API int32_t bert_hip_test_sparse_vocab_geometry(int32_t H, int32_t V, int32_t T, int32_t ns, int32_t max_len, int32_t *geometry);
/* The form and grid bert_hip_test_attention's matrix-core launch (impl 0) takes on the current device for n_sentences sentences of at
 * most max_len tokens (kernels.h attention_mfma_grid; reads the device's CU count): returns the grid, *threads 256 (one workgroup per
 * (sentence, head) item) or 512 (the persistent form: a workgroup walks items grid apart), *items = n_sentences n_head.  0, and zeros,
 * for a shape the launcher refuses; -1 for bad arguments or no device.                                                            */
BERT_API int32_t bert_hip_test_attention_grid(int32_t n_sentences, int32_t n_head, int32_t d_head, int32_t max_len, int32_t *threads,
                                              int32_t *items);
/* How the sparse index's scan cuts a chunk of nq queries with this k over n_rows rows of an index of this dtype and n_vocab
 * (sparse_index_kernels.h sparse_scan_geometry, the function the search itself calls; no GPU): geometry = {qb, n_qtiles, n_slices,
 * slice_rows, L, lds} — queries per tile, tiles, slices of rows, rows per slice (the last may be shorter), entries of a query's LDS list,
 * bytes of LDS per workgroup.  0; -2 and zeros where the plan refuses (dtype outside 0 .. 1, n_vocab outside 1 .. 262144 or, for dtype 1,
 * beyond 65536, n_rows < 0, nq < 1, k outside 1 .. 256); -1 for a NULL geometry.                                                     */
BERT_API int32_t bert_hip_test_sparse_scan_geometry(int32_t dtype, int32_t n_vocab, int32_t n_rows, int32_t nq, int32_t k, int64_t *geometry);
/* The same plan with the tile the tuning key "sparse_index_qb" asks for: qb 1 .. 8 is the tile to aim for, any other value the table's,
 * as bert_hip_set_option reads the key.  What comes back in geometry[0] is what the scan gets: at most nq, and at most what the LDS takes. */
BERT_API int32_t bert_hip_test_sparse_scan_geometry_qb(int32_t dtype, int32_t n_vocab, int32_t n_rows, int32_t nq, int32_t k, int32_t qb,
                                                       int64_t *geometry);
/* How the embedding index's search cuts a chunk of nq queries (1 .. 4096, the queries of one internal pass) with this k over n_rows rows
 * (index.cpp plan, the function the search itself calls; no GPU): geometry = {n_qtiles, n_slices, slice_rows, L} — tiles of 32 queries,
 * slices of rows, rows per slice (a multiple of the 128 rows of a step; the last may be shorter), entries of a query's LDS list.  0; -2 and
 * zeros for n_rows < 0, nq outside 1 .. 4096 or k outside 1 .. 256; -1 for a NULL geometry.                                        */
BERT_API int32_t bert_hip_test_index_plan(int32_t n_rows, int32_t nq, int32_t k, int32_t *geometry);
/* The checks bert_hip_sparse_index_load runs on a file (sparse_index_file.h; the format is in bert_hip.h), without a device.
 * _header: buf holds the first buf_len bytes of a file of file_bytes bytes; 0 and fields = {version, dtype, n_vocab, width, n_rows,
 * has_live} for a header this build loads, -1 and the reason in err (err_cap bytes) otherwise.  _body: fields as _header returned
 * them and the body_len bytes of the file behind its header; 0 if every count, every used id and the live words pass, -1 and the
 * reason in err otherwise (a body_len that is not what the fields describe included).                                            */
BERT_API int32_t bert_hip_test_sparse_index_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err,
                                                   int32_t err_cap);
BERT_API int32_t bert_hip_test_sparse_index_body(const uint32_t *fields, const void *body, int64_t body_len, char *err, int32_t err_cap);
/* How a hybrid search chunks nq queries over indexes of n_rows rows (sparse_index_kernels.h hybrid_chunk_queries, the function the
 * search itself calls; no GPU): out = {HC, ld} — queries per chunk and floats per query of the dense score matrix (n_rows rounded up to
 * 64).  pref: the value of the tuning key "hybrid_chunk_queries" (0 = unset).  0; -2 and zeros for n_rows < 0, nq < 1 or pref < 0; -1
 * for a NULL out.                                                                                                                  */
BERT_API int32_t bert_hip_test_hybrid_chunk(int32_t n_rows, int32_t nq, int32_t pref, int64_t *out);
/* How a token index's scan cuts a chunk of nq queries over n_docs documents (token_index_kernels.h token_index_plan, the function the
 * search itself calls; no GPU): plan = {n_slices, slice_docs} — slice s is documents s slice_docs .. min(n_docs, (s + 1) slice_docs) - 1,
 * one workgroup per (query, slice); an empty index is one empty slice.  pref: the value of the tuning key "token_index_slices" (0 =
 * planned; 1 .. 4096 = that many slices, never more than documents).  0; -2 and zeros for n_docs < 0, nq < 1 or pref outside 0 .. 4096;
 * -1 for a NULL plan.                                                                                                              */
BERT_API int32_t bert_hip_test_token_index_plan(int32_t n_docs, int32_t nq, int32_t pref, int32_t *plan);
/* The checks bert_hip_late_index_load runs on a file (token_index_file.h; the format is in bert_hip.h "LATE INDEX"), without a device.
 * _header: buf holds the first buf_len bytes of a file of file_bytes bytes; 0 and fields = {version, dim, n_docs, has_live, the low
 * and the high 32 bits of n_tokens} for a header this build loads, -1 and the reason in err (err_cap bytes) otherwise.  _body: fields
 * as _header returned them and the body_len bytes of the file behind its header; 0 if the cumulative lengths and the live words pass
 * (the rows are not looked at), -1 and the reason in err otherwise (a body_len that is not what the fields describe included).      */
BERT_API int32_t bert_hip_test_late_index_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err,
                                                 int32_t err_cap);
BERT_API int32_t bert_hip_test_late_index_body(const uint32_t *fields, const void *body, int64_t body_len, char *err, int32_t err_cap);
/* How the sparse index's inverted search cuts a chunk of nq queries with this k over n_rows rows in segments of seg rows
 * (sparse_index_kernels.h sparse_postings_geometry, the function the search itself calls; no GPU): geometry = {qb, n_qtiles, n_slices,
 * slice_segs, L, max_slices, lds} — queries per tile, tiles, slices, whole segments per slice (the last slice may have fewer), entries of
 * a query's LDS list, the workspace's bound on n_slices, bytes of LDS per workgroup.  qb: the value of the tuning key "sparse_index_qb"
 * (0 = unset).  0; -2 and zeros where the plan refuses (sparse_scan_geometry's reasons, or seg outside 256 .. 16384 or no multiple of
 * 256); -1 for a NULL geometry.                                                                                                   */
BERT_API int32_t bert_hip_test_sparse_postings_geometry(int32_t dtype, int32_t n_vocab, int32_t n_rows, int32_t nq, int32_t k, int32_t seg,
                                                        int32_t qb, int64_t *geometry);
/* One segment of an index's postings back on the host (an index of a context of libbert_test.so).  off [n_vocab + 1]: the segment's
 * offsets; rows / weights [cap]: the first min(cap, total) postings in slot order, the row number inside the segment and the weight
 * (f16 exactly converted); *seg_rows: the segment size the postings were built with.  Returns the segment's term total; -2 without
 * postings or for a segment they do not have; -1 without an index or for a NULL pointer; -3 on a device error.  Blocking.          */
BERT_API int32_t bert_hip_test_sparse_postings_segment(struct bert_hip_sparse_index *ix, int32_t segment, int32_t cap, uint32_t *off,
                                                       int32_t *rows, float *weights, int32_t *seg_rows);

#ifdef __cplusplus
}
#endif

#endif /* BERT_HIP_TEST_H */
