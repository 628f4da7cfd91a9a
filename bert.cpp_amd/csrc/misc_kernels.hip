// misc_kernels.hip — the HBM-bound pieces of the forward pass (gfx950): embedding gather-sum +
// LayerNorm, stand-alone LayerNorm, mean-pool + L2 normalise.  One 64-lane wavefront per token row
// with __shfl_xor reductions; no LDS needed.
#include "device.h"
#include "pool_normalize.h"

#include <algorithm>

namespace bert_hip {

// Element e of row r of an embedding table stored in the model-file layout,
// dequantised to f32 exactly as ggml_get_rows does: f16 -> f32, (q-8)*d, q*d+m.
__device__ __forceinline__ float table_elem(const void *tab, int type, int H, int r, int e) {
    if (type == 0) return ((const float *)tab)[(size_t)r * H + e];
    if (type == 1) return (float)((const half_t *)tab)[(size_t)r * H + e];
    const int bs = type == 2 ? 18 : 20;
    const unsigned char *blk = (const unsigned char *)tab + ((size_t)r * (H / 32) + e / 32) * bs;
    const int i = e & 31;
    const float d = (float)*(const half_t *)blk;
    const unsigned char byte = blk[(type == 2 ? 2 : 4) + (i & 15)];
    const int q = i < 16 ? (byte & 0x0F) : (byte >> 4);
    if (type == 2) return (float)(q - 8) * d;
    const float m = (float)*(const half_t *)(blk + 2);
    return (float)q * d + m;
}

// Two adjacent elements (e, e+1; e even) of row r of a table, dequantised to f32.
__device__ __forceinline__ void table_pair(const void *tab, int type, int H, int r, int e, float &a, float &b) {
    if (type == 0) {
        const float2 v = *(const float2 *)((const float *)tab + (size_t)r * H + e);
        a = v.x; b = v.y;
    } else if (type == 1) {
        const f16x2 v = *(const f16x2 *)((const half_t *)tab + (size_t)r * H + e);
        a = (float)v[0]; b = (float)v[1];
    } else {
        a = table_elem(tab, type, H, r, e);
        b = table_elem(tab, type, H, r, e + 1);
    }
}

// reference bert.cpp:796-814: inpL = word[ids]; inpL = type[0] + inpL; inpL = pos[0..N-1] + inpL;
// LayerNorm (ggml_norm eps 1e-5) then gamma * x + beta.  One wave per token, one pass: the row is
// held in registers as NJ element pairs per lane (H <= 128 * NJ, H even).
// max_len (<= the position table's rows: the host refuses a larger one): a token at or behind place max_len of its sentence, which
// only a sentence longer than the device API's promise has, takes row max_len - 1, so the table is never read past its end; what
// its row holds does not matter (the pooling kernel gives that sentence a NaN row).  The same in embed_ln_rows_kernel.
// TYPED (every embedding kernel; bert_hip.h "sentence pairs and scores"): first_len[b] = how many leading tokens of sentence b take row 0
// of the token-type table; a token at a place at or behind it — its place in the sentence, NOT the clamped position row — takes row 1.
// Any value is legal on the device (<= 0: all row 1; >= the length: all row 0, the untyped bits): the row index is a comparison's
// result, 0 or 1.  !TYPED never reads first_len and is the kernel as it was.
template <int NJ, bool TYPED>
__global__ __launch_bounds__(256) void embed_ln_kernel(const void *word, const void *type, const void *pos,
                                                       int table_type, const float *gamma, const float *beta,
                                                       const int32_t *__restrict__ tokens,
                                                       const int32_t *__restrict__ cu_seqlens, int n_sentences,
                                                       int T, int H, int n_vocab, int max_len, half_t *__restrict__ out,
                                                       const int32_t *__restrict__ first_len) {
    // wave-uniform token index: the sentence search below then runs on scalar loads (constant cache)
    const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    // sentence of token t: largest b with cu[b] <= t
    int lo = 0, hi = n_sentences;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu_seqlens[mid] <= t) lo = mid; else hi = mid;
    }
    const int place = t - cu_seqlens[lo], p = min(place, max_len - 1);
    int tr = 0;
    if constexpr (TYPED) tr = place >= first_len[lo] ? 1 : 0;
    int id = tokens[t];
    id = id < 0 ? 0 : (id >= n_vocab ? n_vocab - 1 : id);   // ids are validated on the host API; clamp for safety

    float v[NJ][2];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 2 * lane + 128 * j;
        v[j][0] = v[j][1] = 0.f;
        if (e < H) {
            float w0, w1, t0, t1, p0, p1;
            table_pair(word, table_type, H, id, e, w0, w1);
            table_pair(type, table_type, H, tr, e, t0, t1);
            table_pair(pos, table_type, H, p, e, p0, p1);
            v[j][0] = p0 + (t0 + w0);
            v[j][1] = p1 + (t1 + w1);
            sum += v[j][0] + v[j][1];
        }
    }
    const float mean = wave_sum_f32(sum) / H;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 2 * lane + 128 * j;
        if (e < H) {
            v[j][0] -= mean; v[j][1] -= mean;
            sq += v[j][0] * v[j][0] + v[j][1] * v[j][1];
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum_f32(sq) / H + 1e-5f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 2 * lane + 128 * j;
        if (e < H) {
            f16x2 o;
            o[0] = (_Float16)(gamma[e] * (v[j][0] * rstd) + beta[e]);
            o[1] = (_Float16)(gamma[e + 1] * (v[j][1] * rstd) + beta[e + 1]);
            *(f16x2 *)(out + (size_t)t * H + e) = o;
        }
    }
}

// Same operation for f32 / f16 tables with H % 8 == 0 and q4 tables, laid out for bandwidth: the grid is (4-token group, sentence), so
// a wave knows its sentence and position without searching cu_seqlens; a lane owns 16-byte runs of the row (8
// features: one 16-byte load per f16 table row, one 16-byte store), NC runs per lane (H <= 512 * NC).
template <int TT>
__device__ __forceinline__ void table_run8(const void *tab, int H, int r, int e0, float (&v)[8]) {
    if (TT == 0) {
        const float4 a = *(const float4 *)((const float *)tab + (size_t)r * H + e0);
        const float4 b = *(const float4 *)((const float *)tab + (size_t)r * H + e0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if (TT == 1) {
        const f16x8 h = *(const f16x8 *)((const half_t *)tab + (size_t)r * H + e0);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
    } else {
        // q4_0 / q4_1 rows as stored in the file (18 / 20-byte blocks of 32: d [, m], 16 bytes of nibbles; element j < 16 is the
        // low nibble of byte j, element j + 16 the high one): a run of 8 is one nibble of 8 consecutive bytes.  Same
        // arithmetic as table_elem (ggml_get_rows: (q - 8) d, q d + m in f32).
        constexpr int bs = TT == 2 ? 18 : 20, qo = TT == 2 ? 2 : 4;
        const unsigned char *blk = (const unsigned char *)tab + ((size_t)r * (H / 32) + (e0 >> 5)) * bs;
        const int off = e0 & 31;
        const float d = (float)*(const half_t *)blk;
        const float m = TT == 3 ? (float)*(const half_t *)(blk + 2) : 0.f;
        unsigned short q16[4];                                // (blocks are 2-byte aligned)
#pragma unroll
        for (int i = 0; i < 4; ++i) q16[i] = *(const unsigned short *)(blk + qo + (off & 15) + 2 * i);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int byte = (q16[i >> 1] >> (8 * (i & 1))) & 0xff, q = off < 16 ? (byte & 0x0F) : (byte >> 4);
            v[i] = TT == 2 ? (float)(q - 8) * d : (float)q * d + m;
        }
    }
}
// SEARCH: the grid is (4-token group of the batch) and a wave finds its sentence by bisection of cu_seqlens on scalar loads
// — for batches of short sentences, where the (group, sentence) grid would be mostly empty workgroups.
template <int TT, int NC, bool SEARCH, bool TYPED>
__global__ __launch_bounds__(256) void embed_ln_rows_kernel(const void *word, const void *type, const void *pos,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const int32_t *__restrict__ tokens,
                                                            const int32_t *__restrict__ cu_seqlens, int n_sentences, int T,
                                                            int H, int n_vocab, int max_len, half_t *__restrict__ out,
                                                            const int32_t *__restrict__ first_len) {
    const int lane = threadIdx.x & 63;
    int p = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // position in the sentence / token
    int t, tr = 0;                                            // (tr: the token-type row)
    if constexpr (SEARCH) {
        t = p;
        if (t >= T) return;
        int lo = 0, hi = n_sentences;                         // largest b with cu[b] <= t
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (cu_seqlens[mid] <= t) lo = mid; else hi = mid;
        }
        p = t - cu_seqlens[lo];
        if constexpr (TYPED) tr = p >= first_len[lo] ? 1 : 0;
    } else {
        const int b = blockIdx.y;
        const int tok0 = cu_seqlens[b], n = cu_seqlens[b + 1] - tok0;
        if (p >= n) return;
        t = tok0 + p;
        if constexpr (TYPED) tr = p >= first_len[b] ? 1 : 0;
    }
    p = min(p, max_len - 1);                                  // (the position row; t is settled)
    int id = tokens[t];
    id = id < 0 ? 0 : (id >= n_vocab ? n_vocab - 1 : id);   // ids are validated on the host API; clamp for safety
    float v[NC][8];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int e0 = 8 * (lane + 64 * j);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[j][i] = 0.f;
        if (e0 < H) {
            float w[8], ty[8], ps[8];
            table_run8<TT>(word, H, id, e0, w);
            table_run8<TT>(type, H, tr, e0, ty);
            table_run8<TT>(pos, H, p, e0, ps);
#pragma unroll
            for (int i = 0; i < 8; ++i) { v[j][i] = ps[i] + (ty[i] + w[i]); sum += v[j][i]; }
        }
    }
    const float mean = wave_sum_f32(sum) / H;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (8 * (lane + 64 * j) < H)
#pragma unroll
            for (int i = 0; i < 8; ++i) { v[j][i] -= mean; sq += v[j][i] * v[j][i]; }
    const float rstd = 1.0f / sqrtf(wave_sum_f32(sq) / H + 1e-5f);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int e0 = 8 * (lane + 64 * j);
        if (e0 < H) {
            const float4 g0 = *(const float4 *)(gamma + e0), g1 = *(const float4 *)(gamma + e0 + 4);
            const float4 b0 = *(const float4 *)(beta + e0), b1 = *(const float4 *)(beta + e0 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            f16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (_Float16)(gg[i] * (v[j][i] * rstd) + bb[i]);
            *(f16x8 *)(out + (size_t)t * H + e0) = o;
        }
    }
}

bool launch_embed_ln(const void *word, const void *type, const void *pos, int table_type, const float *gamma,
                     const float *beta, const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, int T,
                     int H, int n_vocab, int max_len, half_t *out, hipStream_t stream, const int32_t *first_len, int form) {
    if (T <= 0) return true;
    const bool rows_shape = (table_type <= 1 ? H % 8 == 0 : H % 32 == 0) && table_type <= 3 && H <= 1024 && max_len > 0;
    if ((form == EMBED_FORM_GRID || form == EMBED_FORM_SEARCH) && !(rows_shape && (form == EMBED_FORM_SEARCH || n_sentences <= GRID_YZ_MAX))) return false;
    if (rows_shape && form != EMBED_FORM_GENERIC) {
        // (group, sentence) grid while at least two thirds of its workgroups have tokens, else one group per 4 tokens
        const bool search = form == EMBED_FORM_AUTO ? n_sentences > GRID_YZ_MAX || 2ll * ((max_len + 3) / 4) * n_sentences > 3ll * ((T + 3) / 4) : form == EMBED_FORM_SEARCH;
        const dim3 g2 = search ? dim3((T + 3) / 4) : dim3((max_len + 3) / 4, n_sentences), b2(256);
#define EMBR_T(TT, NC, SEARCH, TYPED) BERT_LAUNCH((embed_ln_rows_kernel<TT, NC, SEARCH, TYPED>), g2, b2, 0, stream, word, type, pos, gamma, beta, tokens, \
                                                 cu_seqlens, n_sentences, T, H, n_vocab, max_len, out, first_len)
#define EMBR(TT, NC) do { \
            if (search) { if (first_len) EMBR_T(TT, NC, true, true); else EMBR_T(TT, NC, true, false); } \
            else { if (first_len) EMBR_T(TT, NC, false, true); else EMBR_T(TT, NC, false, false); } } while (0)
        if (table_type == 0) { if (H <= 512) EMBR(0, 1); else EMBR(0, 2); }
        else if (table_type == 1) { if (H <= 512) EMBR(1, 1); else EMBR(1, 2); }
        else if (table_type == 2) { if (H <= 512) EMBR(2, 1); else EMBR(2, 2); }
        else { if (H <= 512) EMBR(3, 1); else EMBR(3, 2); }
#undef EMBR
#undef EMBR_T
        return true;
    }
    const dim3 grid((T + 3) / 4), block(256);
    const int nj = (H + 127) / 128;
    const int pos_rows = max_len > 0 ? max_len : T;          // (no promise given: a sentence has at most T tokens)
#define EMB_T(NJ, TYPED) BERT_LAUNCH((embed_ln_kernel<NJ, TYPED>), grid, block, 0, stream, word, type, pos, table_type, gamma, \
                                    beta, tokens, cu_seqlens, n_sentences, T, H, n_vocab, pos_rows, out, first_len)
#define EMB(NJ) do { if (first_len) EMB_T(NJ, true); else EMB_T(NJ, false); } while (0)
    if (nj <= 1) EMB(1); else if (nj <= 3) EMB(3); else if (nj <= 6) EMB(6); else if (nj <= 8) EMB(8); else EMB(32);
#undef EMB
#undef EMB_T
    return true;
}

// The rows kernel's values in LANE ORDER (kernels.h launch_embed_ln_lanes; layer_tail.hip's XRES layout), for model_kernel's full-window
// form: H = 128 NT, T a multiple of 128.  Per token nothing differs from embed_ln_rows_kernel<TT, 1, *> — one wave, lane c owns features
// 8 c .. 8 c + 7, the same sums in the same order, the same clamps: the same bits — but where the 16 bytes go.  A workgroup is a 32-token
// block (8 waves x 4 tokens).  A lane's run of 8 is the halves of two lanes of fragment c >> 1: features 8 c + {0..3} are bytes
// 8 (c & 1) .. of lane (l31, 0), features 8 c + 4 + {0..3} the same bytes of lane (l31, 1).  Stored from registers that would be 8-byte
// scatters; so the block is staged in LDS in fragment order (a KiB + 16 bytes apart: the 8-byte writes of a half wave then fall into
// 32 different bank pairs) and leaves as whole 1 KiB wave-instructions, 16 bytes per lane.
// Sentence and position: block k lies in the 128-token block b = k / 4.  Where sentence b IS that block (cu[b] = 128 b, cu[b + 1] =
// 128 b + 128: every block of a batch of full sentences) the position is t % 128; any other batch of this T — full only by the sum of
// its lengths — bisects cu_seqlens like the SEARCH form, on scalar loads.
template <int TT, int NT, bool TYPED>
__global__ __launch_bounds__(512) void embed_ln_lanes_kernel(const void *word, const void *type, const void *pos,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             const int32_t *__restrict__ tokens,
                                                             const int32_t *__restrict__ cu_seqlens, int n_sentences, int H,
                                                             int n_vocab, int max_len, half_t *__restrict__ xres,
                                                             const int32_t *__restrict__ first_len) {
    constexpr int NQ = 8 * NT, FS = 1024 + 16;                // fragments of a block; bytes from one to the next in LDS
    __shared__ __attribute__((aligned(16))) char S[NQ * FS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tok0 = blockIdx.x * 32, b = tok0 >> 7;
    const bool whole = b < n_sentences && cu_seqlens[b] == 128 * b && cu_seqlens[b + 1] == 128 * b + 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l31 = wave * 4 + i, t = tok0 + l31;
        int p = t & 127, tr = 0;                              // (tr: the token-type row)
        if (!whole) {
            int lo = 0, hi = n_sentences;                     // largest b with cu[b] <= t
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (cu_seqlens[mid] <= t) lo = mid; else hi = mid;
            }
            p = t - cu_seqlens[lo];
            if constexpr (TYPED) tr = p >= first_len[lo] ? 1 : 0;
        } else if constexpr (TYPED) tr = p >= first_len[b] ? 1 : 0;
        p = min(p, max_len - 1);                              // (the position row; t is settled)
        int id = tokens[t];
        id = id < 0 ? 0 : (id >= n_vocab ? n_vocab - 1 : id);   // ids are validated on the host API; clamp for safety
        const int e0 = 8 * lane;
        float v[8];
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = 0.f;
        if (e0 < H) {
            float w[8], ty[8], ps[8];
            table_run8<TT>(word, H, id, e0, w);
            table_run8<TT>(type, H, tr, e0, ty);
            table_run8<TT>(pos, H, p, e0, ps);
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[k] = ps[k] + (ty[k] + w[k]); sum += v[k]; }
        }
        const float mean = wave_sum_f32(sum) / H;
        float sq = 0.f;
        if (e0 < H)
#pragma unroll
            for (int k = 0; k < 8; ++k) { v[k] -= mean; sq += v[k] * v[k]; }
        const float rstd = 1.0f / sqrtf(wave_sum_f32(sq) / H + 1e-5f);
        if (e0 < H) {
            const float4 g0 = *(const float4 *)(gamma + e0), g1 = *(const float4 *)(gamma + e0 + 4);
            const float4 b0 = *(const float4 *)(beta + e0), b1 = *(const float4 *)(beta + e0 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            f16x8 o;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (_Float16)(gg[k] * (v[k] * rstd) + bb[k]);
            char *const d = S + (lane >> 1) * FS + 8 * (lane & 1) + 16 * l31;
            *(f16x4 *)d = f16x4{o[0], o[1], o[2], o[3]};
            *(f16x4 *)(d + 16 * 32) = f16x4{o[4], o[5], o[6], o[7]};
        }
    }
    __syncthreads();
    char *const out = (char *)(xres + (size_t)tok0 * H);
#pragma unroll
    for (int q = wave; q < NQ; q += 8) *(f16x8 *)(out + q * 1024 + lane * 16) = *(const f16x8 *)(S + q * FS + lane * 16);
}

bool embed_ln_lanes_supported(int table_type, int H, int T, int max_len) {
    return T > 0 && T % 128 == 0 && (H == 256 || H == 384) && table_type >= 0 && table_type <= 3 && max_len > 0;
}

bool launch_embed_ln_lanes(const void *word, const void *type, const void *pos, int table_type, const float *gamma,
                           const float *beta, const int32_t *tokens, const int32_t *cu_seqlens, int n_sentences, int T,
                           int H, int n_vocab, int max_len, half_t *xres, hipStream_t stream, const int32_t *first_len) {
    if (!embed_ln_lanes_supported(table_type, H, T, max_len) || n_sentences <= 0) return false;
#define EMBL_T(TT, NT, TYPED) BERT_LAUNCH((embed_ln_lanes_kernel<TT, NT, TYPED>), dim3(T / 32), dim3(512), 0, stream, word, type, pos, gamma, beta, tokens, \
                                          cu_seqlens, n_sentences, H, n_vocab, max_len, xres, first_len)
#define EMBL(TT) do { \
        if (H == 256) { if (first_len) EMBL_T(TT, 2, true); else EMBL_T(TT, 2, false); } \
        else { if (first_len) EMBL_T(TT, 3, true); else EMBL_T(TT, 3, false); } } while (0)
    if (table_type == 0) EMBL(0); else if (table_type == 1) EMBL(1); else if (table_type == 2) EMBL(2); else EMBL(3);
#undef EMBL
#undef EMBL_T
    return true;
}

// reference bert.cpp:868-874 / :894-900 (ggml_norm + gamma/beta), in place on f16 rows.
// NJ = pairs per lane held in registers (H <= 128 * NJ).
template <int NJ>
__global__ __launch_bounds__(256) void layernorm_kernel(half_t *x, const float *gamma, const float *beta, int T, int H) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    half_t *row = x + (size_t)t * H;
    float v[NJ][2];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 2 * lane + 128 * j;
        if (e < H) {
            const f16x2 h2 = *(const f16x2 *)(row + e);
            v[j][0] = (float)h2[0]; v[j][1] = (float)h2[1];
        } else { v[j][0] = 0.f; v[j][1] = 0.f; }
        sum += v[j][0] + v[j][1];
    }
    const float mean = wave_sum_f32(sum) / H;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 2 * lane + 128 * j;
        if (e < H) {
            v[j][0] -= mean; v[j][1] -= mean;
            sq += v[j][0] * v[j][0] + v[j][1] * v[j][1];
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum_f32(sq) / H + 1e-5f);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = 2 * lane + 128 * j;
        if (e < H) {
            f16x2 o;
            o[0] = (_Float16)(gamma[e] * (v[j][0] * rstd) + beta[e]);
            o[1] = (_Float16)(gamma[e + 1] * (v[j][1] * rstd) + beta[e + 1]);
            *(f16x2 *)(row + e) = o;
        }
    }
}

// The same for H % 8 == 0: a lane owns 16-byte runs of the row (one 16-byte load and store per 8 features; the two-byte-pair
// form above moved 2.7 TB/s at H = 768), NC runs per lane (H <= 512 * NC), every run of the row requested before the first is
// touched.  Same arithmetic (two passes, eps 1e-5).  5.1 TB/s at H = 768 and 262 144 rows; two or four rows per wave (more
// loads in flight per lane) measured 0 / +2 % time: the kernel is not short of requests.
template <int NC>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(half_t *x, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, int T, int H) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    half_t *row = x + (size_t)t * H;
    f16x8 h[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int e0 = 8 * (lane + 64 * j);
#pragma unroll
        for (int i = 0; i < 8; ++i) h[j][i] = (_Float16)0.f;
        if (e0 < H) h[j] = *(const f16x8 *)(row + e0);
    }
    float v[NC][8];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) { v[j][i] = (float)h[j][i]; sum += v[j][i]; }
    const float mean = wave_sum_f32(sum) / H;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (8 * (lane + 64 * j) < H)
#pragma unroll
            for (int i = 0; i < 8; ++i) { v[j][i] -= mean; sq += v[j][i] * v[j][i]; }
    const float rstd = 1.0f / sqrtf(wave_sum_f32(sq) / H + 1e-5f);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int e0 = 8 * (lane + 64 * j);
        if (e0 < H) {
            const float4 g0 = *(const float4 *)(gamma + e0), g1 = *(const float4 *)(gamma + e0 + 4);
            const float4 b0 = *(const float4 *)(beta + e0), b1 = *(const float4 *)(beta + e0 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            f16x8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (_Float16)(gg[i] * (v[j][i] * rstd) + bb[i]);
            *(f16x8 *)(row + e0) = o;
        }
    }
}

void launch_layernorm(half_t *x, const float *gamma, const float *beta, int T, int H, hipStream_t stream) {
    if (T <= 0) return;
    if (H % 8 == 0 && H <= 2048) {
        const dim3 grid((T + 3) / 4), block(256);
        if (H <= 512) BERT_LAUNCH(layernorm_rows_kernel<1>, grid, block, 0, stream, x, gamma, beta, T, H);
        else if (H <= 1024) BERT_LAUNCH(layernorm_rows_kernel<2>, grid, block, 0, stream, x, gamma, beta, T, H);
        else BERT_LAUNCH(layernorm_rows_kernel<4>, grid, block, 0, stream, x, gamma, beta, T, H);
        return;
    }
    const dim3 grid((T + 3) / 4), block(256);
    const int nj = (H + 127) / 128;      // H must be even (checked at load)
    if (nj <= 1) BERT_LAUNCH(layernorm_kernel<1>, grid, block, 0, stream, x, gamma, beta, T, H);
    else if (nj <= 3) BERT_LAUNCH(layernorm_kernel<3>, grid, block, 0, stream, x, gamma, beta, T, H);
    else if (nj <= 6) BERT_LAUNCH(layernorm_kernel<6>, grid, block, 0, stream, x, gamma, beta, T, H);
    else if (nj <= 8) BERT_LAUNCH(layernorm_kernel<8>, grid, block, 0, stream, x, gamma, beta, T, H);
    else BERT_LAUNCH(layernorm_kernel<32>, grid, block, 0, stream, x, gamma, beta, T, H);   // H <= 4096
}

// LayerNorm folded into the H = 768 mat-muls (kernels.h GemmLnFold): the residual mat-mul's epilogue left P partial (sum, sum of
// squares) pairs per row; the row's {1 / std, - mean / std, - mean, std} (eps 1e-5) for the mat-muls that read the un-normalised rows
__global__ __launch_bounds__(256) void ln_rows_finalize_kernel(const float2 *__restrict__ stats, int P, int T, float inv_h, float4 *__restrict__ rows) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    float s1 = 0.f, s2 = 0.f;
    for (int p = 0; p < P; ++p) { const float2 v = stats[(size_t)t * P + p]; s1 += v.x; s2 += v.y; }
    const float mean = s1 * inv_h, var = fmaxf(s2 * inv_h - mean * mean, 0.f) + 1e-5f;
    const float sd = sqrtf(var), rstd = 1.0f / sd;
    rows[t] = make_float4(rstd, -mean * rstd, -mean, sd);
}

void launch_ln_rows_finalize(const float2 *stats, int P, int T, int H, float4 *rows, hipStream_t stream) {
    if (T <= 0) return;
    BERT_LAUNCH(ln_rows_finalize_kernel, dim3((T + 255) / 256), dim3(256), 0, stream, stats, P, T, 1.0f / H, rows);
}

// reference bert.cpp:904-913: mean over all N tokens (mat-vec with a 1/N vector), then y / ||y||_2.
// One workgroup per sentence (pool_normalize.h: the body, shared with the epilogue of model_kernel.hip).
__global__ __launch_bounds__(256) void pool_normalize_kernel(const half_t *x, const int32_t *cu_seqlens, int H,
                                                             int max_len, int *status, float *out, int pool_mode) {
    extern __shared__ float part[];          // [4][H] partial sums, then red[4]
    const int b = blockIdx.x;
    const int tok0 = cu_seqlens[b], n = cu_seqlens[b + 1] - tok0;
    pool_normalize_sentence(x, tok0, n, b, H, max_len, status, out, part, (int)threadIdx.x, true, pool_mode);
}

void launch_pool_normalize(const half_t *x, const int32_t *cu_seqlens, int n_sentences, int H, int max_len, int *status,
                           float *out, int pool_mode, hipStream_t stream) {
    if (n_sentences <= 0) return;
    BERT_LAUNCH(pool_normalize_kernel, dim3(n_sentences), dim3(256), (4 * H + 4) * sizeof(float), stream, x,
                       cu_seqlens, H, max_len, status, out, pool_mode);
}

// Grouped pooling (bert_hip.h "long texts"): the un-normalised rows of the sentences group_cu[g] .. group_cu[g + 1] - 1 become ONE row,
// a = (sum_s w_s r_s) / sum_s w_s with w_s = the sentence's token count (cu_seqlens given: the mean over every token state of the
// group) or 1 (cu_seqlens null), divided by its L2 norm unless RAW.  A workgroup per group; thread tid owns elements tid, tid + 256,
// ... of the row and walks the sentences in ascending order with one fmaf chain per element, sum w in integers: no atomics, nothing
// depends on the grid, so a group's bits depend on its own rows and weights alone.  A group of ONE sentence takes its row as it
// stands, and the norm below restates pool_normalize_sentence's reduction (per-thread squares in ascending element order,
// wave_sum_f32, the four partials as (0 + 1) + (2 + 3), 1 / sqrtf): such a group's row is, bit for bit, what the pass gives the
// sentence under the context's own settings.  The un-scaled row waits in `out` itself (a thread reads back only what it wrote), so
// any H >= 1 fits.  A group that is empty, runs backwards or leaves [0, n_sentences] gets a NaN row and sets *status; a NaN row of a
// sentence (one that broke the pass's max_len promise) makes its group's row NaN through the chain.
template <bool RAW>
__global__ __launch_bounds__(256) void group_pool_kernel(const float *__restrict__ rows, const int32_t *__restrict__ cu_seqlens,
                                                         const int32_t *__restrict__ group_cu, int n_sentences, int H, int *status,
                                                         float *out) {
    __shared__ float red[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    const int s0 = group_cu[g], s1 = group_cu[g + 1];
    float *o = out + (size_t)g * H;
    if (s0 < 0 || s1 <= s0 || s1 > n_sentences) {
        for (int e = tid; e < H; e += 256) o[e] = __builtin_nanf("");
        if (tid == 0 && status) atomicOr(status, 1);
        return;
    }
    const bool one = s1 - s0 == 1;                            // (uniform)
    float inv = 0.f;
    if (!one) {
        int wsum = s1 - s0;
        if (cu_seqlens) wsum = cu_seqlens[s1] - cu_seqlens[s0];
        inv = 1.0f / (float)wsum;
    }
    float sq = 0.f;
    for (int e = tid; e < H; e += 256) {
        float a;
        if (one) a = rows[(size_t)s0 * H + e];
        else {
            float acc = 0.f;
            for (int s = s0; s < s1; ++s) {
                const int w = cu_seqlens ? cu_seqlens[s + 1] - cu_seqlens[s] : 1;
                acc = fmaf((float)w, rows[(size_t)s * H + e], acc);
            }
            a = acc * inv;
        }
        o[e] = a;
        if constexpr (!RAW) sq += a * a;
    }
    if constexpr (!RAW) {
        sq = wave_sum_f32(sq);
        if ((tid & 63) == 0) red[tid >> 6] = sq;
        __syncthreads();
        const float scale = 1.0f / sqrtf((red[0] + red[1]) + (red[2] + red[3]));
        for (int e = tid; e < H; e += 256) o[e] = o[e] * scale;
    }
}

void launch_group_pool(const float *rows, const int32_t *cu_seqlens, const int32_t *group_cu, int n_sentences, int n_groups, int H,
                       bool raw, int *status, float *out, hipStream_t stream) {
    if (n_groups <= 0) return;
    if (raw) BERT_LAUNCH(group_pool_kernel<true>, dim3(n_groups), dim3(256), 0, stream, rows, cu_seqlens, group_cu, n_sentences, H, status, out);
    else BERT_LAUNCH(group_pool_kernel<false>, dim3(n_groups), dim3(256), 0, stream, rows, cu_seqlens, group_cu, n_sentences, H, status, out);
}

// Token rows (kernels.h launch_token_rows): the final states of a pass, [T][H] in row order, to the caller's buffer.  One wave per token
// row; a lane owns runs of VW elements (VW = 8 where H % 8 == 0: 16-byte loads of f16 rows; else single elements), run lane + 64 j of the
// row.  S: the stored type (f16, or f32 on the f32 route), O: the output's.  NORM: the row over its L2 norm — a lane adds the squares of
// its elements in ascending order in f32, wave_sum_f32 adds the lanes, scale = 1 / sqrtf(sum), no epsilon (the pooling's rule); the row
// is read a second time (L1 / L2) instead of being kept.  !NORM: the stored value converted, nothing else.  A wave finds its sentence
// by bisection of cu_seqlens on scalar loads; a token of a sentence whose length is not in [1, max_len], or behind the last
// sentence, gets a NaN row.
template <class S, int VW>
__device__ __forceinline__ void token_run_load(const S *p, float (&v)[VW]) {
    if constexpr (VW == 1) v[0] = (float)p[0];
    else if constexpr (std::is_same_v<S, float>) {
        const float4 a = *(const float4 *)p, b = *(const float4 *)(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const f16x8 hv = *(const f16x8 *)p;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)hv[i];
    }
}
template <class O, int VW>
__device__ __forceinline__ void token_run_store(O *p, const float (&v)[VW]) {
    if constexpr (VW == 1) p[0] = (O)v[0];
    else if constexpr (std::is_same_v<O, float>) {
        *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        f16x8 hv;
#pragma unroll
        for (int i = 0; i < 8; ++i) hv[i] = (_Float16)v[i];
        *(f16x8 *)p = hv;
    }
}
template <class S, class O, int VW, bool NORM>
__global__ __launch_bounds__(256) void token_rows_kernel(const S *__restrict__ x, int T, int H, const int32_t *__restrict__ cu_seqlens,
                                                         int n_sentences, int max_len, O *__restrict__ out) {
    const int t = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    int lo = 0, hi = n_sentences;                             // largest b with cu[b] <= t
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu_seqlens[mid] <= t) lo = mid; else hi = mid;
    }
    const int n = cu_seqlens[lo + 1] - cu_seqlens[lo];
    const bool bad = n < 1 || n > max_len || t < cu_seqlens[lo] || t >= cu_seqlens[lo + 1];      // (wave-uniform)
    const S *row = x + (size_t)t * H;
    O *orow = out + (size_t)t * H;
    float scale = 1.f;
    if (NORM && !bad) {
        float sq = 0.f;
        for (int e0 = lane * VW; e0 < H; e0 += 64 * VW) {
            float v[VW];
            token_run_load<S, VW>(row + e0, v);
#pragma unroll
            for (int i = 0; i < VW; ++i) sq += v[i] * v[i];
        }
        scale = 1.0f / sqrtf(wave_sum_f32(sq));
    }
    for (int e0 = lane * VW; e0 < H; e0 += 64 * VW) {
        float v[VW];
        if (bad) {
#pragma unroll
            for (int i = 0; i < VW; ++i) v[i] = __builtin_nanf("");
        } else {
            token_run_load<S, VW>(row + e0, v);
            if (NORM) {
#pragma unroll
                for (int i = 0; i < VW; ++i) v[i] = v[i] * scale;
            }
        }
        token_run_store<O, VW>(orow + e0, v);
    }
}

void launch_token_rows(const void *x, bool x_is_f32, int T, int H, const int32_t *cu_seqlens, int n_sentences, int max_len, int flags,
                       void *out, hipStream_t stream) {
    if (T <= 0 || n_sentences <= 0) return;
    const dim3 grid((T + 3) / 4), block(256);
    const bool norm = flags & TOKEN_ROWS_NORMALIZE, o16 = flags & TOKEN_ROWS_F16, vec = H % 8 == 0;
#define TOKR(S, O, VW, NORM) BERT_LAUNCH((token_rows_kernel<S, O, VW, NORM>), grid, block, 0, stream, (const S *)x, T, H, cu_seqlens, n_sentences, max_len, (O *)out)
#define TOKR_N(S, O, VW) do { if (norm) TOKR(S, O, VW, true); else TOKR(S, O, VW, false); } while (0)
#define TOKR_V(S, O) do { if (vec) TOKR_N(S, O, 8); else TOKR_N(S, O, 1); } while (0)
    if (x_is_f32) { if (o16) TOKR_V(float, half_t); else TOKR_V(float, float); }
    else { if (o16) TOKR_V(half_t, half_t); else TOKR_V(half_t, float); }
#undef TOKR_V
#undef TOKR_N
#undef TOKR
}

// A call's staged block (ids | cu_seqlens | windows) from MAPPED pinned host memory into device memory by a kernel: the copy
// engine needs about 20 us before the first kernel behind it can start, a few workgroups reading 16 bytes per lane across the host
// link need 5-8 for the 130 KB of a 256 x 128 batch (engine.hip eval_packed_host; small blocks only).
__global__ __launch_bounds__(256) void stage_copy_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int n16) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) dst[i] = src[i];
}

// Both blocks must hold `bytes` rounded up to 16.  The one caller, Engine::eval_packed_host, sizes its pinned block and its device
// image at in_bytes + 16, in_bytes being the sum of the three parts of the largest chunk, each rounded up to 16 (so a multiple of
// 16 itself), and copies off_w + 8 n_windows <= in_bytes bytes (build_windows makes at most one window a sentence): the last whole
// unit ends at or before in_bytes.
void launch_stage_copy(const void *mapped_src, void *dst, size_t bytes, hipStream_t stream) {
    const int n16 = (int)((bytes + 15) / 16);
    if (n16 <= 0) return;
    BERT_LAUNCH(stage_copy_kernel, dim3(std::min(64, (n16 + 255) / 256)), dim3(256), 0, stream, (const uint4 *)mapped_src, (uint4 *)dst, n16);
}

__global__ void f16_to_f32_kernel(const half_t *src, float *dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

void launch_f16_to_f32(const half_t *src, float *dst, size_t n, hipStream_t stream) {
    if (!n) return;
    BERT_LAUNCH(f16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, dst, n);
}

}  // namespace bert_hip
