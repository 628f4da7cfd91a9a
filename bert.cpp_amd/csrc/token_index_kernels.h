// token_index_kernels.h — the device code of the token index (token_index.hip, token_index_grouped.hip) as its host side
// (token_index.cpp) sees it: the three stored forms and the table that states them (TOKEN_FORMS), the plan of a scan, the argument
// blocks and the launchers — one for the ten instantiations of the two scan kernels, one for the quantisers, one each for the pairs
// and the gather kernel.  A launcher only enqueues: the caller reads hipGetLastError.  dtype is the index's: 1 f16, 2 int8, 4 mxfp4.
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
// Stored form, mxfp4 (bert_hip.h "TOKEN INDEX, MXFP4 form").  uint8 rows[n_tokens][token_mx_row_bytes(dim)] and the same cu: per token
// the embedding index's mxfp4 row — dpad / 2 bytes of e2m1 codes (dpad = dim rounded up to a multiple of 64, the padding zero), dpad / 32
// E8M0 scale bytes (one per 32 elements), zero bytes to a multiple of 16 — by device.h's quantize_row_mx; no array beside the rows.
// Queries are quantised per token to MXFP8 rows of token_mx_query_bytes(dim) bytes (dpad e4m3 codes, the same scale bytes, padded to
// 16) into the same [nq][max_q_len] workspace.  A row or query token with a NaN or +-inf: codes 0, every scale byte 0xFF.
//
// A scan workgroup (token_index_scan_kernel, one kernel with a form per dtype) stages one query in LDS as ceil(n / 32) blocks of 32 rows
// padded by 16 bytes, what else its form keeps beside them, then a list of L (score, id) entries and a count: token_scan_lds_bytes.
// The grouped scan of the f16 form (token_index_scan_grouped_kernel) stages up to four queries that way: token_group_lds_bytes.
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
__host__ __device__ inline int token_mx_dpad(int dim) { return (dim + 63) & ~63; }
__host__ __device__ inline size_t token_mx_row_bytes(int dim) { return mx_row_bytes(token_mx_dpad(dim) >> 1, token_mx_dpad(dim)); }
__host__ __device__ inline size_t token_mx_query_bytes(int dim) { return mx_row_bytes(token_mx_dpad(dim), token_mx_dpad(dim)); }
// the mxfp4 form's staged query row: the MXFP8 row, and one more 16-byte slot where its slots come out even (an odd count of slots
// puts the 32 rows of a ds_read_b128 step on distinct slots of the bank row: 9 at dim 128, 25 at 384, 50 + 1 at 768, 66 + 1 at 1024)
__host__ __device__ inline int token_mx_ldq(int dim) { const int slots = (int)(token_mx_query_bytes(dim) >> 4); return 16 * (slots | 1); }
inline size_t token_f16_row_bytes(int dim) { return (size_t)dim * 2; }
inline size_t token_i8_row_bytes(int dim) { return (size_t)token_i8_dpad(dim); }
// What a form stages per query token: a row of dim + 8 halfs (maxsim's padding), of dpad + 16 bytes of codes (the same 16 bytes), or
// of token_mx_ldq bytes (the mxfp4 form: codes and scale bytes in one row)
inline size_t token_f16_lds_row_bytes(int dim) { return (size_t)(dim + 8) * 2; }
inline size_t token_i8_lds_row_bytes(int dim) { return (size_t)token_i8_dpad(dim) + 16; }
inline size_t token_mx_lds_row_bytes(int dim) { return (size_t)token_mx_ldq(dim); }

// What the quantisers write (launch_token_quantize): the int8 form's codes and scales — stored rows and queries alike —, the mxfp4
// form's stored rows, or the MXFP8 rows its queries take
enum TokenQuant { TOKEN_QUANT_NONE = -1, TOKEN_QUANT_I8, TOKEN_QUANT_MXFP4, TOKEN_QUANT_MXFP8 };
// bytes of a row of such a target, and whether one f32 scale per row goes into an array beside the rows
constexpr size_t (*TOKEN_QUANT_ROW_BYTES[3])(int dim) = {token_i8_row_bytes, token_mx_row_bytes, token_mx_query_bytes};
inline bool token_quant_scales(TokenQuant t) { return t == TOKEN_QUANT_I8; }

// Everything the host knows of a stored form, one row per dtype: the place a new form starts.  The device side of a form is its Form
// in token_index.hip and its entries in that file's list of scan instantiations
struct TokenForm {
    int dtype;
    const char *name;                           // for messages
    int dpad_step;                              // dpad = dim rounded up to a multiple of this (f16: no kernel reads it; the int8 form's)
    size_t (*row_bytes)(int dim);               // a stored row
    // what an add quantises to (its scales beside the rows) and what a search's queries become in the workspace; NONE, both: the rows
    // are stored as they come and the scan reads the caller's
    TokenQuant rows, queries;
    size_t (*lds_row_bytes)(int dim);           // a query token staged in LDS
    size_t lds_extra;                           // LDS beside the query's blocks (int8: the query's scales)
    bool has_file;                              // compact and the file form exist
    // the profiler's names: the scan plain and masked; the grouped scan likewise (null: chunks of this form are never grouped); the
    // LISTED scan as a rescore (null: a rescore is token_index_pairs_kernel and maxsim); the quantiser (null: none)
    const char *scan[2], *grouped[2], *rescore, *quantize;
};
constexpr TokenForm TOKEN_FORMS[3] = {
    {1, "f16", 32, token_f16_row_bytes, TOKEN_QUANT_NONE, TOKEN_QUANT_NONE, token_f16_lds_row_bytes, 0, true,
     {"token_index_scan", "token_index_scan_masked"}, {"token_index_scan_grouped", "token_index_scan_grouped_masked"}, nullptr, nullptr},
    {2, "int8", 32, token_i8_row_bytes, TOKEN_QUANT_I8, TOKEN_QUANT_I8, token_i8_lds_row_bytes, TOKEN_MAX_QUERY * 4, false,
     {"token_i8_scan", "token_i8_scan_masked"}, {nullptr, nullptr}, "token_i8_rescore", "token_i8_quantize"},
    {4, "mxfp4", 64, token_mx_row_bytes, TOKEN_QUANT_MXFP4, TOKEN_QUANT_MXFP8, token_mx_lds_row_bytes, 0, false,
     {"token_mxfp4_scan", "token_mxfp4_scan_masked"}, {nullptr, nullptr}, "token_mxfp4_rescore", "token_mx_quantize"},
};
// the row of dtype, null for a dtype that is no form
inline const TokenForm *token_form(int dtype) {
    for (const TokenForm &f : TOKEN_FORMS)
        if (f.dtype == dtype) return &f;
    return nullptr;
}
inline int token_dpad(const TokenForm &f, int dim) { return (dim + f.dpad_step - 1) / f.dpad_step * f.dpad_step; }

// a staged block of 32 tokens, and what the form keeps beside the blocks
inline size_t token_query_block_bytes(int dim, int dtype) { return (size_t)TOKEN_QB * token_form(dtype)->lds_row_bytes(dim); }
inline size_t token_query_extra_bytes(int dtype) { return token_form(dtype)->lds_extra; }
// the query's blocks, the form's extra bytes, the list (8 L bytes), the count (16)
inline size_t token_scan_lds_bytes(int dim, int dtype, int max_q_len, int k) {
    return (size_t)token_query_blocks(max_q_len) * token_query_block_bytes(dim, dtype) + token_query_extra_bytes(dtype) + (size_t)token_list_L(k) * 8 + 16;
}
// the largest multiple of 32, at most TOKEN_MAX_QUERY, whose blocks fit TOKEN_LDS_MAX beside the longest list.  f16: dim <= 384: 128,
// <= 768: 96, <= 1024: 64.  int8: 128 at every dim (dim 1024, 128 tokens, the longest list: 137 744 bytes).  mxfp4: 128 at every dim
// (dim 1024: rows of 1072 bytes, 141 328 bytes with the longest list)
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

// The grouped scan of the f16 form (token_index_grouped.hip): one workgroup serves G consecutive queries over one slice and loads every
// document block once for all of them.  Every query of a group gets ceil(max_q_len / 32) block slots (the host knows the launch's
// max_q_len, not the lengths), then G lists of L entries and their counts
constexpr int TOKEN_MAX_GROUP = 4;
inline size_t token_group_lds_bytes(int dim, int max_q_len, int k, int g) {
    return (size_t)g * (token_query_blocks(max_q_len) * token_query_block_bytes(dim, 1) + (size_t)token_list_L(k) * 8) + 16;
}
// The planned G (the key at 0), from profiles/token_group_rate.txt (tools/token_group_rate.py: 10^6 x 25 and 10^5 x 180 tokens, dim 384 and
// 128, 32-token queries, 1 / 8 / 64 queries): a cell's fastest arm where it beat key 1 by more than the cell's min .. max spread, else 1.
// dim 384: key 3 in all four cells of 8 and 64 queries (0.95, 0.78, 0.61, 0.52 of key 1's time; key 4, one workgroup a CU, behind it).
// dim 128: key 4 over the long documents (0.62, 0.63) but key 1 over the short ones (key 4: 1.11, 1.09 of its time), and the plan does
// not know the documents' lengths: 1.  One query: 1.  Not measured: 2 .. 7 queries (1), dims between the two (1) and above 384 (3, which
// the LDS cuts to 2 at dim 1024: their rows are longer still)
inline int token_group_planned(int dim, int nq) { return dim >= 384 && nq >= 8 ? 3 : 1; }
// G of a chunk of nq queries: the largest value that is at most TOKEN_MAX_GROUP, at most nq, at most the tuning key
// "token_index_query_group" (key: 1 = never group, 2 .. 4 = at most that many; 0 = token_group_planned) and whose LDS fits
// TOKEN_LDS_MAX.  1 = the ungrouped kernel, which a form without a grouped scan launches whatever the key.  With 32-token queries the LDS allows 4 at
// dim <= 384, 3 at 768, 2 at 1024; with 128-token queries at dim 384: 1.  The one place this is decided: the search and the test hook
// call it, reserve bounds it by token_group_cap
inline int token_query_group(int dim, int dtype, int max_q_len, int nq, int k, int key) {
    if (!token_form(dtype)->grouped[0] || nq < 2 || key == 1) return 1;
    int g = std::min({TOKEN_MAX_GROUP, nq, key >= 2 ? key : token_group_planned(dim, nq)});
    while (g > 1 && token_group_lds_bytes(dim, max_q_len, k, g) > TOKEN_LDS_MAX) --g;
    return g;
}
// the most queries a group of any later search may hold under this key (reserve's workspace bound: max_q_len and k may be smaller then)
inline int token_group_cap(int dtype, int key) { return !token_form(dtype)->grouped[0] || key == 1 ? 1 : key >= 2 ? std::min(key, TOKEN_MAX_GROUP) : TOKEN_MAX_GROUP; }

// token_index_scan_kernel, every form.  LDS: token_scan_lds_bytes(dim, dtype, max_q_len, k)
struct TokenScanArgs {
    const void *rows;                   // the index: half_t [n_tokens][dim], int8 codes [n_tokens][dpad], or mxfp4 rows [n_tokens][token_mx_row_bytes]
    const float *scales = nullptr;      // int8: [n_tokens]
    const int32_t *cu;                  // [n_docs + 1]
    const void *q;                      // f16: the queries' rows, indexed by qcu.  int8: the queries' workspace, codes [nq][max_q_len][dpad]
                                        // mxfp4: the workspace of MXFP8 rows [nq][max_q_len][token_mx_query_bytes]
    const float *q_scales = nullptr;    // int8: [nq][max_q_len]
    const int32_t *qcu;                 // [nq + 1]
    float *ws_s;                        // [nq][n_slices][k] per-(query, slice) lists, best first
    int *ws_i;
    int n_docs, dim, dpad, nq, max_q_len, n_slices, slice_docs, k, L, n_items;
    // the masked instantiation (either non-null): words [ceil(n_docs / 32)], bit d & 31 of word d >> 5 set = document d is live / may
    // be returned; a null pointer = all ones.  No word at or beyond ceil(n_docs / 32) is read
    const uint32_t *live = nullptr;
    const uint32_t *allow = nullptr;
    // the listed instantiation (cand non-null; int8 and mxfp4): a rescore.  The "documents" of a slice are positions of the query's candidate
    // list cand[qi][0 .. n_cand), n_cand takes n_docs' place in the plan, and live is tested per id (allow is not used)
    const int32_t *cand = nullptr;      // [nq][n_cand]
    int n_cand = 0;
};

// token_index_scan_grouped_kernel (f16 form; cand, n_cand, scales and q_scales are not used): the scan's arguments with nq queries in
// n_groups groups of `group` consecutive queries (the last group holds what is left), n_items = n_slices * n_groups, item = slice *
// n_groups + group index.  The workspace is the ungrouped scan's, [nq][n_slices][k].  LDS: token_group_lds_bytes(dim, max_q_len, k, group)
struct TokenGroupScanArgs : TokenScanArgs {
    int group = 1, n_groups = 0;
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

// token_i8_quantize_kernel and token_mx_quantize_kernel: rows of dim values (f32 or f16: f16 is converted exactly) -> a TokenQuant's
// rows, one wave per row, by device.h's quantize_row_i8 (codes to dst, scales beside them) or quantize_row_mx (scales null).
// qcu == nullptr: rows src[0 .. n) -> rows 0 .. n - 1 of dst / scales.  qcu != nullptr (the queries of a search): n = nq * max_q_len
// slots; slot qi * max_q_len + t takes row qcu[qi] + t of src where the query passes the scan's guards (not empty, not descending, not
// starting below 0, at most max_q_len tokens) and t is below its length, and is left alone otherwise: no row outside a query's range is read
struct TokenQuantizeArgs {
    const void *src;
    void *dst;
    float *scales;
    long long n;
    int dim, dpad;
    const int32_t *qcu = nullptr;
    int max_q_len = 0;
};

// token_index_grouped.hip's entries of token_index.hip's list of scan instantiations: its kernel plain [0] and masked [1]
using TokenGroupScanKernel = void (*)(TokenGroupScanArgs);
const TokenGroupScanKernel *token_scan_grouped_kernels();
// lets every scan instantiation of the current device have TOKEN_LDS_MAX of LDS
void token_index_kernels_init();
// One scan of dtype's form: the grouped kernel where a.group >= 2 (f16, a search), else token_index_scan_kernel — listed if a.cand is
// set (int8 and mxfp4), else masked if a.live or a.allow is, else plain.  token_scan_label: the profiler's name of that launch
const char *token_scan_label(int dtype, const TokenGroupScanArgs &a);
void launch_token_scan(int dtype, const TokenGroupScanArgs &a, hipStream_t s);
// (target: not NONE; src_f32: the rows are f32, else f16; more rows than one launch takes go in several)
void launch_token_quantize(TokenQuant target, const TokenQuantizeArgs &a, bool src_f32, hipStream_t s);
void launch_token_pairs(const TokenPairsArgs &a, hipStream_t s);
void launch_token_gather(const TokenGatherArgs &a, hipStream_t s);

}  // namespace bert_hip
