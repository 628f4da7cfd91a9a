// token_index_kernels.h — the device code of the token index (token_index.hip) as its host side (token_index.cpp) sees it: the two
// stored forms, the plan of a scan, the argument blocks and one launcher per kernel.  A launcher only enqueues: the caller reads
// hipGetLastError.  dtype is the index's: 1 f16, 2 int8.
//
// Stored form, f16.  half_t rows[n_tokens][dim], packed, 16-byte aligned (dim a multiple of 8 in 8 .. MAXSIM_MAX_H), and int32
// cu[n_docs + 1]: document d is rows cu[d] .. cu[d + 1] - 1, never empty — what maxsim.hip takes as its document side, so a rescore
// hands the index's own arrays to launch_maxsim.
//
// Stored form, int8 (bert_hip.h "TOKEN INDEX, int8 form").  int8 codes[n_tokens][dpad] (dpad = dim rounded up to a multiple of 32, the
// padding zero, rows 16-byte aligned), float scales[n_tokens] and the same cu.  A row x is scale = amax / 127 and
// code_i = clamp(rint(x_i / scale), -127, 127) — device.h's quantize_row_i8, the embedding index's rule: all codes 0 where the scale is 0;
// scale NaN and codes 0 where an element is NaN or +-inf.  Queries are quantised the same way, per token, into a workspace of
// [nq][max_q_len] rows (query qi's token t at row qi * max_q_len + t), so the scan finds a query's rows without its neighbours' lengths.
//
// A scan workgroup (token_index_scan_kernel, one kernel with a form per dtype) stages one query in LDS as ceil(n / 32) blocks of 32 rows
// padded by 16 bytes, what else its form keeps beside them, then a list of L (score, id) entries and a count: token_scan_lds_bytes.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "search_kernels.h"

namespace bert_hip {

constexpr int TOKEN_QB = 32;                            // query tokens of a block: the B side of one 32 x 32 MFMA block
constexpr int TOKEN_MAX_QUERY = 128;                    // the longest query a search takes at any dim
constexpr int TOKEN_ROUNDS = 16;                        // documents a wave scores between two looks at the list
constexpr int TOKEN_STEP_DOCS = NWAVE * TOKEN_ROUNDS;   // the most entries a workgroup pushes between two looks
// a planned slice is at least four documents per wave: long against the query it stages and the k entries it hands to the merge, short
// enough that 10^5 documents still make TARGET_BLOCKS workgroups (at 64 they made 1562: one and a half rounds of the 1024 a chip holds)
constexpr int TOKEN_MIN_SLICE_DOCS = 4 * NWAVE;
constexpr int TOKEN_MAX_SLICES = 4096;                  // the tuning key's range
constexpr int TOKEN_MAX_CAND = 1024;
// the dynamic LDS a scan workgroup may ask for: the CU's 160 KiB less a margin for what the compiler allocates statically
constexpr size_t TOKEN_LDS_MAX = 160 * 1024 - 256;

// entries of the LDS list: the top-k ahead of a queue that takes a step's pushes
inline int token_list_L(int k) { return k + TOKEN_STEP_DOCS <= 256 ? 256 : 512; }
inline int token_query_blocks(int n) { return (n + TOKEN_QB - 1) / TOKEN_QB; }
inline int token_i8_dpad(int dim) { return (dim + 31) & ~31; }
// What a form stages per query.  A block of 32 tokens: rows of dim + 8 halfs (maxsim's padding), or of dpad + 16 bytes of codes (the
// same 16 bytes).  Beside the blocks: nothing, or the int8 form's 512 bytes of query scales
inline size_t token_query_block_bytes(int dim, int dtype) { return (size_t)TOKEN_QB * (dtype == 2 ? token_i8_dpad(dim) + 16 : (dim + 8) * 2); }
inline size_t token_query_extra_bytes(int dtype) { return dtype == 2 ? TOKEN_MAX_QUERY * 4 : 0; }
// the query's blocks, the form's extra bytes, the list (8 L bytes), the count (16)
inline size_t token_scan_lds_bytes(int dim, int dtype, int max_q_len, int k) {
    return (size_t)token_query_blocks(max_q_len) * token_query_block_bytes(dim, dtype) + token_query_extra_bytes(dtype) + (size_t)token_list_L(k) * 8 + 16;
}
// the largest multiple of 32, at most TOKEN_MAX_QUERY, whose blocks fit TOKEN_LDS_MAX beside the longest list.  f16: dim <= 384: 128,
// <= 768: 96, <= 1024: 64.  int8: 128 at every dim (dim 1024, 128 tokens, the longest list: 137 744 bytes)
inline int token_max_query_tokens(int dim, int dtype) {
    const size_t room = TOKEN_LDS_MAX - token_query_extra_bytes(dtype) - (size_t)512 * 8 - 16;
    return (int)std::min<size_t>(TOKEN_MAX_QUERY, room / token_query_block_bytes(dim, dtype) * TOKEN_QB);
}

// How a chunk of nq queries over n_docs documents is cut into workgroups of token_index_scan_kernel: one workgroup per (query, slice
// of slice_docs consecutive documents), TARGET_BLOCKS workgroups aimed for, equal counts per slice (the last takes what is left), no
// planned slice shorter than TOKEN_MIN_SLICE_DOCS.  pref (the tuning key "token_index_slices", 1 .. TOKEN_MAX_SLICES; 0 = planned):
// that many slices instead, never more than documents.  An empty index is one empty slice.  The one place this is decided: the search,
// reserve and the test hook all call it.  (max_slices: what n_slices never exceeds for these nq and pref however n_docs grows up to
// the n_docs given — the workspace bound)
struct TokenScanPlan { int n_slices, slice_docs, max_slices; };
inline bool token_index_plan(int n_docs, int nq, int pref, TokenScanPlan &p) {
    p = TokenScanPlan{0, 0, 0};
    if (n_docs < 0 || nq < 1 || pref < 0 || pref > TOKEN_MAX_SLICES) return false;
    const int aim = pref > 0 ? std::min(pref, std::max(n_docs, 1))
                             : std::max(1, std::min((TARGET_BLOCKS + nq - 1) / nq, n_docs / TOKEN_MIN_SLICE_DOCS));
    p.max_slices = aim;
    p.slice_docs = std::max(1, (int)(((long long)n_docs + aim - 1) / aim));
    p.n_slices = std::max(1, (int)(((long long)n_docs + p.slice_docs - 1) / p.slice_docs));
    return true;
}

// token_index_scan_kernel, both forms.  LDS: token_scan_lds_bytes(dim, dtype, max_q_len, k)
struct TokenScanArgs {
    const void *rows;                   // the index: half_t [n_tokens][dim], or int8 codes [n_tokens][dpad]
    const float *scales = nullptr;      // int8: [n_tokens]
    const int32_t *cu;                  // [n_docs + 1]
    const void *q;                      // f16: the queries' rows, indexed by qcu.  int8: the queries' workspace, codes [nq][max_q_len][dpad]
    const float *q_scales = nullptr;    // int8: [nq][max_q_len]
    const int32_t *qcu;                 // [nq + 1]
    float *ws_s;                        // [nq][n_slices][k] per-(query, slice) lists, best first
    int *ws_i;
    int n_docs, dim, dpad, nq, max_q_len, n_slices, slice_docs, k, L, n_items;
    // the masked instantiation (either non-null): words [ceil(n_docs / 32)], bit d & 31 of word d >> 5 set = document d is live / may
    // be returned; a null pointer = all ones.  No word at or beyond ceil(n_docs / 32) is read
    const uint32_t *live = nullptr;
    const uint32_t *allow = nullptr;
    // the listed instantiation (cand non-null; int8 only): a rescore.  The "documents" of a slice are positions of the query's candidate
    // list cand[qi][0 .. n_cand), n_cand takes n_docs' place in the plan, and live is tested per id (allow is not used)
    const int32_t *cand = nullptr;      // [nq][n_cand]
    int n_cand = 0;
};

// token_index_pairs_kernel: cand [nq][n_cand] -> maxsim's pair list pairs [nq * n_cand][2] = (q, id), and ws_i [nq][n_cand] = id; an
// id outside [0, n_docs), or one whose bit of live (nullable, as the scan's) is clear, becomes the pair (q, -1) — which launch_maxsim
// scores NaN without reading a row — and the id INT_MAX
struct TokenPairsArgs {
    const int32_t *cand;
    int32_t *pairs;
    int *ws_i;
    int nq, n_cand, n_docs;
    const uint32_t *live = nullptr;
};

// token_index_gather_kernel (compaction): document j of the n kept ones is document old_ids[j] of src — its rows src_cu[old_ids[j]] ..
// go to rows dst_cu[j] .. dst_cu[j + 1] - 1 of dst, in 16-byte pieces.  old_ids [n], src_cu (the old lengths) and dst_cu [n + 1] in
// device memory; the lengths agree (dst_cu is built from src_cu on the host)
struct TokenGatherArgs {
    const half_t *src;
    half_t *dst;
    const int32_t *src_cu, *dst_cu, *old_ids;
    int n, dim;
};

// token_i8_quantize_kernel: rows of dim values (f32 or f16: f16 is converted exactly) -> codes and scales, one wave per row.
// qcu == nullptr: rows src[0 .. n) -> rows 0 .. n - 1 of codes / scales.  qcu != nullptr (the queries of a search): n = nq * max_q_len
// slots; slot qi * max_q_len + t takes row qcu[qi] + t of src where the query passes the scan's guards (not empty, not descending, not
// starting below 0, at most max_q_len tokens) and t is below its length, and is left alone otherwise: no row outside a query's range is read
struct TokenI8QuantizeArgs {
    const void *src;
    int8_t *codes;
    float *scales;
    long long n;
    int dim, dpad;
    const int32_t *qcu = nullptr;
    int max_q_len = 0;
};

// lets every scan instantiation of the current device have TOKEN_LDS_MAX of LDS
void token_index_kernels_init();
// the instantiation of dtype's form: listed if a.cand is set (int8 only), else masked if a.live or a.allow is, else plain
void launch_token_scan(int dtype, const TokenScanArgs &a, hipStream_t s);
// (src_f32: the rows are f32, else f16; more rows than one launch takes go in several)
void launch_token_i8_quantize(const TokenI8QuantizeArgs &a, bool src_f32, hipStream_t s);
void launch_token_pairs(const TokenPairsArgs &a, hipStream_t s);
void launch_token_gather(const TokenGatherArgs &a, hipStream_t s);

}  // namespace bert_hip
