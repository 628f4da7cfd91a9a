// kernels.h — launch interface of the HIP kernels of the bert_eval hot path (gfx950 only): the weight layouts, the launch_*
// functions and the launch bookkeeping host code needs.  The device-side building blocks the kernels share are in device.h.
//
// Reference ops each kernel replaces are listed in SURVEY.md §2.3; call sites bert.cpp:796-913.
// Activations are f16 row-major [T_pad][features]; T_pad is T rounded up to GEMM_BM tokens.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cstdint>
#include <thread>

namespace bert_hip {

typedef _Float16 half_t;

constexpr int GEMM_BM = 128;   // token tile
constexpr int GEMM_BN = 128;   // feature tile
constexpr int GEMM_BK = 64;    // reduction tile (two 32-weight quant blocks)

// What the launches assume grid.y and grid.z hold on every device (the least the programming model promises; DESIGN.md §3 has what
// the MI355X's runtime reports): a launch whose y or z could exceed it goes in slices.
constexpr int GRID_YZ_MAX = 65535;

enum Epilogue : int { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESID = 2 };
enum GemmWType : int { GW_F16 = 0, GW_Q4_0 = 1, GW_Q4_1 = 2 };

// A weight matrix W[N][K] (out-features x in-features) in its HBM layout.
//   GW_F16 : w16  [N_pad][K] f16 row-major (rows N..N_pad are zero)
//   GW_Q4_x: qs   one uint4 (16 B of nibbles) per 32-weight block, tile-contiguous:
//                 index = ((nt * (K/64) + kt) * 128 + row_in_tile) * 2 + block_in_ktile
//            sc   f16 scale per block (q4_0) or f16x2 {d, m} per block (q4_1), same order
//   naive16: optional f16 [N][K] row-major dequantised copy used by the generic fallback kernel
struct GemmWeight {
    int N = 0, K = 0, N_pad = 0;
    int type = GW_F16;
    const half_t *w16 = nullptr;
    const uint4 *qs = nullptr;
    const void *sc = nullptr;
    const half_t *naive16 = nullptr;
    // optional second f16 image whose k order inside every group of 16 is [0-3, 8-11, 4-7, 12-15]: a 16-byte half
    // of a group then holds the k's one lane of an MFMA accumulator column owns (layer_tail.hip)
    const half_t *w16p = nullptr;
    // f32 files (ftype 0) with the f32 route (f32_route.hip): the file's own f32 rows, [N][K] row-major
    const float *w32 = nullptr;
};

// C[t][n] = epi( sum_k A[t][k] * W[n][k] + bias[n] (+ resid[t][n]) ), t < M_pad (multiple of 128)
// lda = K, ldc = ldr = N.  MFMA path requires K % 64 == 0.
void launch_gemm_mfma(const GemmWeight &W, const half_t *A, const float *bias, const half_t *resid, half_t *C,
                      int M_pad, int epilogue, hipStream_t stream);
// Large-tile variant (gemm256.hip): 256 x 256 x 64 tiles, 8 waves; f16 weights, N % 256 == 0, M_pad % 256 == 0.
bool gemm256_supported(const GemmWeight &W, int M_pad);
// LayerNorm folded into the mat-muls around it (H = 768 route; reference bert.cpp:866-875, :892-901 have it as operations of their
// own): a residual mat-mul writes the UN-normalised sum u (f16) and per-row partial statistics of it (STATS); ln_rows_finalize turns
// those into {rstd, -mean rstd, -mean, std} per row; a mat-mul that consumes LayerNorm(u) reads u itself with gamma folded into its
// weights and ONE extra k-step that carries - mean s[n] + std c[n] (s = row sums of the folded weights, c = W beta + bias), its
// epilogue multiplying by rstd (IN); a residual mat-mul whose residual is LayerNorm(u) rebuilds it per element from u, the row
// statistics and packed (gamma, beta + bias) pairs (RES).  f16 images only.
struct GemmLnFold {
    enum : int { IN = 1, RES = 2, STATS = 4 };
    int flags = 0;
    const float4 *rows_in = nullptr;      // IN: statistics of A's rows
    const half_t *waug = nullptr;         // IN: [N][16] f16 weight side of the statistics k-step
    const float4 *rows_res = nullptr;     // RES: statistics of resid's rows
    const unsigned *gb = nullptr;         // RES: [N] f16 gamma | f16 (beta + bias) << 16
    float2 *stats = nullptr;              // STATS: [M_pad][2 N / 256] (sum, sum of squares)
};
// false, launching nothing: a LayerNorm-folding form (ln->flags set) that no kernel runs — a matrix that is not an f16 image, or
// an (epilogue, flags) pair other than (EPI_BIAS | EPI_BIAS_GELU, IN), (EPI_BIAS_RESID, STATS), (EPI_BIAS_RESID, RES | STATS)
bool launch_gemm256(const GemmWeight &W, const half_t *A, const float *bias, const half_t *resid, half_t *C, int M_pad,
                    int epilogue, hipStream_t stream, const GemmLnFold *ln = nullptr);
// per-row partial statistics [T][P] -> {rstd, -mean rstd, -mean, std} (eps 1e-5, H features per row)
void launch_ln_rows_finalize(const float2 *stats, int P, int T, int H, float4 *rows, hipStream_t stream);
// Out-projection + LN + FFN + LN in one launch (layer_tail.hip): a pair of specialist waves per 32 tokens (up-projection +
// GELU / down-projection); H = 256 / 384; f16 weights (W1 / W2 need w16p) or q4 planes.
bool layer_tail_supported(const GemmWeight &Wo, const GemmWeight &W1, const GemmWeight &W2);
void launch_layer_tail(const GemmWeight &Wo, const GemmWeight &W1, const GemmWeight &W2, const half_t *ctx, const half_t *x,
                       const float *bo, const float *g1, const float *be1, const float *b1, const float *b2,
                       const float *g2, const float *be2, half_t *out, int M_pad, hipStream_t stream);
// All encoder layers of a batch in one launch (model_kernel.hip): a workgroup carries its window (whole sentences, at most 128
// tokens between them) through every layer — the window kernel's and the layer tail's bodies as phases, same bits.
constexpr int MODEL_MAX_LAYERS = 12;       // (the layers' pointers travel in the kernel's argument block)
struct ModelLayerWeights {
    const GemmWeight *Wqkv, *Wo, *W1, *W2;
    const float *bqkv, *bo, *g1, *be1, *b1, *b2, *g2, *be2;
};
bool model_kernel_supported(const GemmWeight &Wqkv, const GemmWeight &Wo, const GemmWeight &W1, const GemmWeight &W2, int n_layer,
                            int n_head, int d_head, int max_len);
// x: in = embeddings + LayerNorm (the ragged form; the full form reads none), out = the last layer's output; ctx: workspace [T][H] (the
// ragged form's); xres: workspace [T][H] (full windows: in = embeddings + LayerNorm in lane order, launch_embed_ln_lanes; then the residual
// between the layers' tails in the same order; no other route's data survives in it).  groups / n_groups / n_groups_dev: the
// window list as for launch_qkv_attention2 (nullptr: one sentence per window); n_tokens = 128 n_sentences selects the form
// specialised for full windows.  pooled != nullptr: the workgroups also pool and normalise their sentences (launch_pool_normalize's
// arguments and bits: [n_sentences][H] f32, max_len, status word, pool_mode).
void launch_model_kernel(const ModelLayerWeights *layers, int n_layer, half_t *x, half_t *ctx, half_t *xres, const int32_t *cu_seqlens, int n_sentences,
                         int n_tokens, const int2 *groups, int n_groups, const int *n_groups_dev, int n_head, float *pooled, int max_len,
                         int *status, int pool_mode, int slots, hipStream_t stream);
// The latency route (skinny.hip): the weight mat-muls of a layer split by output features AND token blocks over up to 192
// one-wave workgroups, for batches of at most 128 tokens; same bits per sentence as qkv_attention2 + layer_tail.
// mode: 0 QKV projection (-> f16), 1 out-projection (+ x + bo -> f32), 2 up-projection + GELU (-> f16, fragment order),
// 3 down-projection (+ y + b2 -> f32).  V != nullptr (modes 0, 2): the kernel LayerNorms the f32 rows V itself (gamma, beta)
// and writes them to ln_out; else A holds the f16 token rows.  n_token_blocks = ceil(T / 32) <= 4.
bool skinny_layer_supported(const GemmWeight &Wqkv, const GemmWeight &Wo, const GemmWeight &W1, const GemmWeight &W2);
void launch_skinny_gemm(int mode, const GemmWeight &W, const half_t *A, const float *V, const float *gamma, const float *beta,
                        half_t *ln_out, const float *bias, const half_t *resid, half_t *out16, float *out32, int n_token_blocks,
                        hipStream_t stream);
// the last layer's LayerNorm 2: f32 rows -> f16 rows
void launch_skinny_layernorm(const float *v, const float *gamma, const float *beta, half_t *out, int n_token_blocks, int H,
                             hipStream_t stream);
// Generic fallback (any K, N); needs W.naive16.
void launch_gemm_naive(const GemmWeight &W, const half_t *A, const float *bias, const half_t *resid, half_t *C,
                       int M, int epilogue, hipStream_t stream);

// form (the op-level tests pick one; the engine leaves the choice to the launcher): the rows kernel on its (group, sentence) grid or
// with the bisection, or the generic kernel.  A rows form on a shape the rows kernel does not take launches nothing: false.
enum : int { EMBED_FORM_AUTO = -1, EMBED_FORM_GRID = 0, EMBED_FORM_SEARCH = 1, EMBED_FORM_GENERIC = 2 };
// word + token_type + position gather-sum, LayerNorm(eps 1e-5), f16 out.  Tables in file layout.
// max_len (the device API's promise, <= the position table's rows): chooses the grid form; no position row at or behind it is read.
// first_len (all four embedding launchers; device memory, [n_sentences], nullable): the leading tokens of sentence b that take
// token-type row 0, every token at a place at or behind it row 1 — the place in the sentence, not the clamped position row.  Any value
// is legal (<= 0: all row 1, >= the length: all row 0).  Null: row 0 for every token, on the kernels' untyped instantiations.
bool launch_embed_ln(const void *word, const void *type, const void *pos, int table_type, const float *gamma,
                     const float *beta, const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, int T,
                     int H, int n_vocab, int max_len, half_t *out, hipStream_t stream, const int32_t *first_len = nullptr,
                     int form = EMBED_FORM_AUTO);
// The same values in LANE ORDER, for launch_model_kernel's full-window form, which starts from them in `xres` and reads no rows: block k
// (tokens 32 k .. 32 k + 31) is the 32 H halves from 32 k H on, fragment q < H / 16 its KiB q, lane l = 32 hi + l31 owns 16 bytes at 16 l
// of it: features 16 q + 4 hi + {0..3}, then 16 q + 8 + 4 hi + {0..3} of token 32 k + l31 (layer_tail.hip's XRES layout).  Its shapes:
// T a positive multiple of 128, H = 256 or 384, table types 0..3, max_len >= 1; any other is refused — false, nothing launched.
bool embed_ln_lanes_supported(int table_type, int H, int T, int max_len);
bool launch_embed_ln_lanes(const void *word, const void *type, const void *pos, int table_type, const float *gamma,
                           const float *beta, const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, int T,
                           int H, int n_vocab, int max_len, half_t *xres, hipStream_t stream, const int32_t *first_len = nullptr);

// In-place LayerNorm over H of f16 rows (eps 1e-5), gamma/beta f32.
void launch_layernorm(half_t *x, const float *gamma, const float *beta, int T, int H, hipStream_t stream);

// qkv [T_pad][3H] (Q | K | V), packed sentences; out ctx [T_pad][H].
// MFMA path supports d_head in {32, 64}; returns false if the shape needs the naive kernel.
// rel, P: a relative position bias (MPNet), score(i, j) = <q_i, k_j> / sqrt(d_head) + bias[h][j - i]; rel [n_head][2 P - 1] f32 on the
// device is weights.h rel_bias_table for sentences of up to P tokens — for the MFMA kernel times sqrt(d_head) (it scales the sum), for
// the naive kernel the bias itself.  nullptr: no bias, the kernels every pass without one runs.
bool launch_attention_mfma(const half_t *qkv, const int32_t *cu_seqlens, int n_sentences, int n_head, int d_head,
                           int max_len, half_t *out, hipStream_t stream, const float *rel = nullptr, int P = 0);
void launch_attention_naive(const half_t *qkv, const int32_t *cu_seqlens, int n_sentences, int n_head, int d_head,
                            int max_len, half_t *out, hipStream_t stream, const float *rel = nullptr, int P = 0);
// The form and grid launch_attention_mfma launches on the current device: threads per workgroup — 256, one workgroup per (sentence, head)
// item, up to 128 tokens; 512, the persistent form, beyond: min(CUs / 8 * 8, items / 8 * 8) workgroups (all of fewer than 8 items) that
// walk the items —, the grid and the items.  All zero where the launcher refuses the shape (d_head, or more LDS than 160 KiB; bias: a
// launch with a relative position bias, which keeps 8 bytes per key slot more).
struct AttentionGrid { int threads, grid, items; };
AttentionGrid attention_mfma_grid(int n_sentences, int n_head, int d_head, int max_len, bool bias = false);

// Q|K|V projection + attention in one kernel (qkv_attention2.hip): x [T_pad][H] -> ctx [T_pad][H].  A workgroup owns a window
// of 128 token slots holding one or several whole sentences (16-slot aligned); f16 or q4 weights, d_head 32, H = 128 / 256 / 384, every sentence <= 128 tokens.
// `groups` [n_groups] = {first sentence, count} per window (device memory), or nullptr: the uniform rule
// 128 / round_up(max_len, 16) sentences per window.
bool qkv_attention2_supported(const GemmWeight &Wqkv, int n_head, int d_head, int max_len);
int qkv_attention2_sentences_per_window(int max_len, int slots);
// n_groups_dev (optional): device word with the real number of windows when `groups` was built on the device and n_groups is
// only an upper bound (launch_build_windows / qkv_attention2_max_windows).
void launch_qkv_attention2(const GemmWeight &Wqkv, const half_t *x, const float *bias, const int32_t *cu_seqlens,
                           int n_sentences, const int2 *groups, int n_groups, const int *n_groups_dev, int max_len, int n_head,
                           int slots, half_t *out, hipStream_t stream);
// next-fit windows (the rule of Engine::build_windows) computed on the device from cu_seqlens; *n_windows receives their number
void launch_build_windows(const int32_t *cu_seqlens, int n_sentences, int2 *windows, int *n_windows, int slots, hipStream_t stream);
int qkv_attention2_max_windows(int n_sentences, int n_tokens, int slots);
// place granularity of the windows (16, or 8: qkv_attention2.hip): the process-wide default; every function above takes the
// value its caller read once per forward pass (`slots`)
int window_slots();
void set_window_slots(int slots);

// How a pass ends (bert_hip.h "pooling" / "normalize"), the bits of every `pool_mode` below: 0 = mean over the sentence's tokens, then
// L2 normalise (the reference's); POOL_CLS: the row of the sentence's first token instead of the mean; POOL_RAW: no division by the norm.
constexpr int POOL_CLS = 1, POOL_RAW = 2;
// the sentences' rows by that rule; out f32 [n_sentences][H].  A sentence whose length is not in [1, max_len] (the caller of the
// device API promised max_len) gets a NaN row and sets *status (device word) to 1, whatever the mode.
void launch_pool_normalize(const half_t *x, const int32_t *cu_seqlens, int n_sentences, int H, int max_len, int *status,
                           float *out, int pool_mode, hipStream_t stream);

// Grouped pooling (bert_hip.h "long texts"; misc_kernels.hip): rows f32 [n_sentences][H], the sentences' POOL_RAW rows of a pass;
// group g = sentences group_cu[g] .. group_cu[g + 1] - 1 (device memory, n_groups + 1 entries); out f32 [n_groups][H], not the rows'
// memory: the weighted mean of the group's rows — weights the sentences' token counts from cu_seqlens, or 1 each when cu_seqlens is
// null —, divided by its L2 norm unless raw.  A group of one sentence: the bits launch_pool_normalize gives that sentence without
// POOL_RAW.  A group that is empty, not ascending or outside [0, n_sentences] gets a NaN row and sets *status to 1.  Any H >= 1.
void launch_group_pool(const float *rows, const int32_t *cu_seqlens, const int32_t *group_cu, int n_sentences, int n_groups, int H,
                       bool raw, int *status, float *out, hipStream_t stream);

// Token rows (bert_hip.h "token rows and late interaction"; misc_kernels.hip): the final states x [T][H] of a pass in row order — f16,
// or f32 (x_is_f32: the f32 route's) — copied to out [T][H], one wave per row.  flags bit 0 (TOKEN_ROWS_NORMALIZE): every row divided
// by its own L2 norm (f32 sum of squares, a lane's elements in ascending order, then wave_sum_f32; 1 / sqrtf, no epsilon); bit 1
// (TOKEN_ROWS_F16): out is f16 (rounded to nearest even), else f32.  Without bit 0 the f32 output is the stored state exactly.  The
// tokens of a sentence whose length is not in [1, max_len] get NaN rows (the pooling launch sets the status word for it).  Any H >= 1.
// One launch of a 256-thread workgroup per four tokens: T <= TOKEN_ROWS_MAX_T keeps it at 2^31 threads (the host forms cut their
// passes at "chunk_tokens" and tokenized calls hold fewer tokens than that; bert_hip_eval_packed_tokens_device refuses more).
constexpr int TOKEN_ROWS_NORMALIZE = 1, TOKEN_ROWS_F16 = 2, TOKEN_ROWS_MAX_T = 1 << 25;
void launch_token_rows(const void *x, bool x_is_f32, int T, int H, const int32_t *cu_seqlens, int n_sentences, int max_len, int flags,
                       void *out, hipStream_t stream);

// MaxSim (maxsim.hip): q [.][H], d [.][H] packed f16 token rows, 16-byte aligned, H % 8 == 0, 8 <= H <= MAXSIM_MAX_H; qcu [n_q + 1],
// dcu [n_d + 1] cumulative lengths; pairs null: all pairs, scores [n_q][n_d]; else [n_pairs][2] of (a, b), scores [n_pairs].
// mode bit 0: the mean over the query tokens instead of the sum.  Everything in device memory.
// One workgroup of 256 threads serves one pair, and a launch of 2^32 threads or more is not run as asked: launch_maxsim cuts the pairs
// into launches of at most MAXSIM_LAUNCH_PAIRS (256 threads each: 2^31 threads), `first` being a launch's first pair (the launcher's
// field: callers leave it 0).  launch_pairs (the tuning key "maxsim_launch_pairs"): fewer pairs per launch, 1 .. MAXSIM_LAUNCH_PAIRS;
// 0 = that bound.  A pair's bits depend on its own rows alone, so no result depends on the cut.
constexpr int MAXSIM_MAX_H = 1024;
constexpr int MAXSIM_LAUNCH_PAIRS = 1 << 23;
struct MaxsimArgs {
    const half_t *q, *d;
    const int32_t *qcu, *dcu, *pairs;
    float *scores;
    int n_q, n_d, H, n_pairs, mode;
    long long first;
};
size_t maxsim_lds_bytes(int H);
// The classification head (cls_head.hip; bert_hip.h "sentence pairs and scores"): rows f32 [B][H], the sentences' POOL_CLS | POOL_RAW rows
// of a pass -> out f32 [B][n_labels] = Wc tanh(Wp row + bp) + bc, n_labels in 1 .. CLS_HEAD_MAX_LABELS.  wp16: Wp [H][H] f16 row-major
// (row = out-feature), 16-byte aligned; wp32: the same as f32 (f32 files).  bp [H], wc [n_labels][H], bc [n_labels]: f32.
// flags bit 0 (CLS_HEAD_SIGMOID): 1 / (1 + exp(-logit)) per label instead of the logit.
// launch_cls_head: the matrix-core form (H % 8 == 0, 8 <= H <= CLS_HEAD_MFMA_MAX_H; wp16) — false, nothing launched, for another H.
// launch_cls_head_f32: one workgroup per sentence, f32 dot products; Wp from wp32 if given, else wp16; false for H > 8192.
constexpr int CLS_HEAD_MAX_LABELS = 8, CLS_HEAD_MFMA_MAX_H = 1024, CLS_HEAD_SIGMOID = 1;
struct ClsHeadArgs {
    const float *rows;
    const half_t *wp16;
    const float *wp32, *bp, *wc, *bc;
    float *out;
    int B, H, n_labels, flags;
};
bool cls_head_mfma_supported(int H);
size_t cls_head_lds_bytes(int H);
bool launch_cls_head(const ClsHeadArgs &a, hipStream_t stream);
bool launch_cls_head_f32(const ClsHeadArgs &a, hipStream_t stream);
// Learned sparse weights (sparse_vocab.hip; bert_hip.h "learned sparse embeddings"): t [T][H], the MLM transform of a pass's packed token
// rows; e [V][H], the tied vocabulary matrix, row-major; bias [V] f32; cu [n_sentences + 1] cumulative lengths (device memory), of
// which sentences s0 .. s0 + ns - 1 are served: out f32 [ns][V],
//   out[b][v] = z > 0 ? log1pf(z) : +0,  z = (max over the tokens i of sentence s0 + b of <t_i, e_v>) + bias[v].
// No token row at or behind T and no vocabulary row at or behind V is read.  max_len: the longest sentence the caller promises (it
// bounds the grid; tokens of a longer sentence behind that bound do not enter).
// launch_sparse_vocab: the matrix-core form — t16 / e16 f16, 16-byte aligned, H % 8 == 0, 8 <= H <= SPARSE_MFMA_MAX_H; the products are
// score_chain_f16's.  It zero-fills out itself (hipMemsetAsync), combines the pieces of a sentence that spans token tiles by an integer
// atomic max on the bits of the non-negative z (exact and commutative: no bit depends on the order of arrival), and applies log1pf in
// place by a second launch, sparse_finish.  false, nothing enqueued, for another H.
// launch_sparse_vocab_f32: the plain form, any H — f32 fmaf chains over k = lane, lane + 64, ..., wave_sum_f32; operands t32 / e32
// (f32) where given, else t16 / e16; one workgroup per (sentence, 64 vocabulary entries), plain stores.
constexpr int SPARSE_MFMA_MAX_H = 1024;
struct SparseVocabArgs {
    const half_t *t16, *e16;
    const float *t32, *e32, *bias;
    const int32_t *cu;
    float *out;
    int s0, ns, T, H, V, max_len;
};
bool sparse_vocab_mfma_supported(int H);
size_t sparse_vocab_lds_bytes(int H);
bool launch_sparse_vocab(const SparseVocabArgs &a, hipStream_t stream);       // the vocabulary launch alone (out: the bits of relu(z))
// The grid launch_sparse_vocab launches for a shape, host arithmetic alone: `tile` token slots per workgroup (128, or 64 above H = 624),
// n_tiles of them over min(T, ns max_len) tokens (grid.x), vocabulary slabs of slab_blocks 32-entry blocks — a multiple of 8 in 8 .. 64 —
// and n_slabs of them (grid.y).  false, and zeros, exactly where the launcher refuses the shape.
struct SparseVocabGeometry { int tile, n_tiles, slab_blocks, n_slabs; };
bool sparse_vocab_geometry(int H, int V, int T, int ns, int max_len, SparseVocabGeometry &g);
void launch_sparse_finish(float *out, size_t n, hipStream_t stream);          // log1pf in place
bool launch_sparse_vocab_f32(const SparseVocabArgs &a, hipStream_t stream);
// Top-k terms of dense rows w [n][V] (sparse_vocab.hip): per row the k largest POSITIVE weights, larger first, equal weights smaller id
// first; ids [n][k] (-1 in unused places), weights [n][k] (+0 there).  1 <= k <= SPARSE_MAX_K, V < 2^24.  One workgroup per row.
constexpr int SPARSE_MAX_K = 256;
bool launch_sparse_topk(const float *w, int n, int V, int k, int32_t *ids, float *weights, hipStream_t stream);
void launch_maxsim(const MaxsimArgs &a, hipStream_t stream, int launch_pairs = 0);
// n f32 values -> f16, rounded to nearest even (the host form of MaxSim rounds its rows on the device).  One thread per value in one
// launch: n <= F32_TO_F16_MAX_N (2^31 threads), which the callers see to
constexpr size_t F32_TO_F16_MAX_N = (size_t)1 << 31;
void launch_f32_to_f16(const float *src, half_t *dst, size_t n, hipStream_t stream);

// The > 64 KiB dynamic-LDS opt-in (hipFuncSetAttribute) is per device: `seen` is the launcher's per-kernel record.  The
// devices of a context launch from threads of their own, and two contexts may share a device: the record is atomic, and
// the first launcher on a device finishes the opt-in (`mark_configured`) before anybody else launches past it.
constexpr int MAX_HIP_DEVICES = 64;
typedef std::atomic<int> DeviceFlags[MAX_HIP_DEVICES];        // 0 = not configured, 1 = being configured, 2 = done
inline int current_device_slot() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d & (MAX_HIP_DEVICES - 1);
}
// true for exactly one caller per device: it runs the opt-in and then calls mark_configured(); everybody else waits for that
inline bool first_launch_on_device(DeviceFlags &seen) {
    std::atomic<int> &f = seen[current_device_slot()];
    int expected = 0;
    if (f.load(std::memory_order_acquire) == 2) return false;
    if (f.compare_exchange_strong(expected, 1, std::memory_order_acq_rel)) return true;
    while (f.load(std::memory_order_acquire) != 2) std::this_thread::yield();
    return false;
}
inline void mark_configured(DeviceFlags &seen) { seen[current_device_slot()].store(2, std::memory_order_release); }
template <class F>
inline void configure_once(DeviceFlags &seen, F &&opt_in) {
    if (first_launch_on_device(seen)) { opt_in(); mark_configured(seen); }
}

// Every kernel of the path is launched through BERT_LAUNCH.  While the engine profiles (Engine::timed) the launching thread
// points tl_launch_timing at an event pair and the launch goes through hipExtLaunchKernelGGL, which attaches the events to the
// dispatch itself (no hipEventRecord barrier packets of their own in the stream).  Measured (round 4): a launch timed alone
// still reads long — model_kernel 825-866 us against 780 us in rocprofv3's trace of the same steps — whatever the events'
// fence flags; for kernels of a millisecond and more the two agree within 1 %.  These times feed the per-kernel BREAKDOWN; the
// roofline's kernel time comes from replay groups (profiler.h timed(), bench.py kernel_roofline).
// `launches` counts the launches a timed body issued: the event pair is only meaningful for exactly one (a body that returns
// without launching leaves stale timestamps in pooled events, a body with two launches measures the last one).
struct LaunchTiming { hipEvent_t start, stop; int launches; };
inline thread_local LaunchTiming *tl_launch_timing = nullptr;
#define BERT_LAUNCH(kernel, grid, block, lds, stream, ...)                                                                     \
    do {                                                                                                                      \
        if (::bert_hip::tl_launch_timing) {                                                                                   \
            ++::bert_hip::tl_launch_timing->launches;                                                                         \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ::bert_hip::tl_launch_timing->start,                      \
                                  ::bert_hip::tl_launch_timing->stop, 0, __VA_ARGS__);                                        \
        } else hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                             \
    } while (0)

// The XCD item map of the kernels whose consecutive items share data (the query tiles of one slice of rows): workgroup b runs on
// XCD b % 8, so item (b % 8) * (grid / 8) + b / 8 sends consecutive items to one XCD, where they find the slice in that XCD's L2.
// The grid is a multiple of 8 — xcd_grid, the launch side — and a workgroup whose item is at or beyond n_items does nothing.
__device__ __forceinline__ int xcd_item() { return (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8); }
inline int xcd_grid(int n_items) { return (n_items + 7) / 8 * 8; }

// The f32 route (f32_route.hip): the forward pass of f32 model files in f32 arithmetic — f32 activations, mat-muls on
// v_mfma_f32_32x32x2_f32 (any M, N, K; C = epi(A W^T + bias (+ resid))), f32 softmax / GELU / LayerNorm / pooling.
void launch_f32_embed_ln(const float *word, const float *type, const float *pos, const float *gamma, const float *beta, const int32_t *tokens,
                         const int32_t *cu_seqlens, int n_sentences, int T, int H, int n_vocab, int max_len, float *out, hipStream_t stream,
                         const int32_t *first_len = nullptr);
void launch_f32_gemm(const float *A, const float *W, const float *bias, const float *resid, float *C, int M, int N, int K, int epilogue,
                     hipStream_t stream);
// One wave per query keeps its max_len scores in LDS, four waves a workgroup: f32_attention_lds_bytes(max_len) = 64 ceil(max_len / 4)
// bytes of dynamic LDS.  false, and NO launch, when that exceeds f32_attention_lds_limit(), what the current device's properties give a
// workgroup (sharedMemPerBlock), or when max_len < 1.
size_t f32_attention_lds_bytes(int max_len);
size_t f32_attention_lds_limit();
// rel, P: as launch_attention_naive (the bias itself).
bool launch_f32_attention(const float *qkv, const int32_t *cu_seqlens, int n_sentences, int n_head, int d_head, int max_len, float *out,
                          hipStream_t stream, const float *rel = nullptr, int P = 0);
void launch_f32_layernorm(float *x, const float *gamma, const float *beta, int T, int H, hipStream_t stream);
void launch_f32_pool_normalize(const float *x, const int32_t *cu_seqlens, int n_sentences, int H, int max_len, int *status, float *out,
                               int pool_mode, hipStream_t stream);

// bytes (rounded up to 16) from mapped pinned host memory to device memory by a kernel (small staged blocks of the host API)
void launch_stage_copy(const void *mapped_src, void *dst, size_t bytes, hipStream_t stream);

// f16 [rows][cols] -> f32 (hidden-state tap)
void launch_f16_to_f32(const half_t *src, float *dst, size_t n, hipStream_t stream);

}  // namespace bert_hip
