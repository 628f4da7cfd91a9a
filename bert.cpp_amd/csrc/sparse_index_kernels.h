// sparse_index_kernels.h — the device code of the sparse index (sparse_index.hip) as its host side (sparse_index.cpp) sees it: the
// stored form, the query image, the plan of a scan, the argument blocks and one launcher per kernel.  dtype is the index's: 0 = i32 ids
// and f32 weights, 1 = u16 ids and f16 weights.  A launcher only enqueues: the caller reads hipGetLastError.
//
// Stored form (sliced ELL).  Rows live in blocks of SPARSE_BLOCK_ROWS = 64, one wavefront per block; inside a block the layout is
// column-major, ids[block][j][lane] and weights[block][j][lane] for j < width, in two arrays.  A row's terms stand in columns
// 0 .. count - 1 in ascending id, the columns behind hold id 0 and weight +0; counts[row] is the row's term count.  A wave reads column
// j of its 64 rows as one coalesced access and every lane owns one row and one fma chain in j order.
//
// Query image: what the scan reads from LDS for one query — a bitmap over the vocabulary (words = ceil(n_vocab / 32) u32), one u16
// count of the set bits below each word, and the weights in rank (ascending id) order, SPARSE_MAX_TERMS f32 — img_bytes each, a
// multiple of 16.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "search_kernels.h"

namespace bert_hip {

constexpr int SPARSE_BLOCK_ROWS = 64;
constexpr int SPARSE_MAX_TERMS = 256;                   // terms of a row (width) and of a query (kq), at most
constexpr int SPARSE_MAX_VOCAB = 262144;
constexpr int SPARSE_STEP_ROWS = SPARSE_BLOCK_ROWS * NWAVE;     // rows a scan workgroup scores per step (each wave one block)
// entries of a query's LDS list: the top-k ahead of a queue that takes at least half a step more than one step's rows
inline int sparse_list_L(int k) { return k <= 128 ? 512 : 1024; }
constexpr int SPARSE_MIN_SLICE_ROWS = 2048;             // a slice is long against the k entries it hands to the merge
// the dynamic LDS a scan workgroup may ask for: the CU's 160 KiB less a margin for what the compiler allocates statically (the
// workgroup reductions behind __syncthreads_or)
constexpr size_t SPARSE_LDS_MAX = 160 * 1024 - 256;
constexpr int SPARSE_QB_MAX = 8;                        // the most queries of a tile: a lane keeps an accumulator and a threshold pair for each
constexpr int SPARSE_QB[2] = {2, 2};                    // queries per tile the scan aims for, by dtype

inline size_t sparse_id_bytes(int dtype) { return dtype == 1 ? 2 : 4; }
inline int sparse_image_words(int n_vocab) { return (n_vocab + 31) / 32; }
// the parts of a query image: words u32 | words u16, padded to 4 bytes | SPARSE_MAX_TERMS f32, the whole padded to 16 bytes
inline size_t sparse_image_bytes(int n_vocab) {
    const size_t w = (size_t)sparse_image_words(n_vocab);
    return (w * 4 + ((w * 2 + 3) & ~(size_t)3) + (size_t)SPARSE_MAX_TERMS * 4 + 15) & ~(size_t)15;
}

// How a chunk of nq queries over n_rows rows is cut into workgroups of sparse_index_scan_kernel: tiles of qb queries times slices of
// slice_rows rows (a multiple of SPARSE_STEP_ROWS, so every slice starts at a block), and a workgroup's LDS — qb query images, then
// per query a list of L = sparse_list_L(k) (score, id) entries and a count.  The one place this is decided: the launcher's caller and the
// test hook both call it.  qb_pref: 0, or the tile to aim for in place of SPARSE_QB (the tuning key "sparse_index_qb").
// (max_slices: what n_slices never exceeds, and what never falls as n_rows grows — the workspace bound)
struct SparseScanGeometry { int qb, n_qtiles, n_slices, slice_rows, L, max_slices; size_t lds; };
inline bool sparse_scan_geometry(int dtype, int n_vocab, int n_rows, int nq, int k, SparseScanGeometry &g, int qb_pref = 0) {
    g = SparseScanGeometry{0, 0, 0, 0, 0, 0, 0};
    if (dtype < 0 || dtype > 1 || n_vocab < 1 || n_vocab > SPARSE_MAX_VOCAB || (dtype == 1 && n_vocab > 65536) || n_rows < 0 || nq < 1 ||
        k < 1 || k > SPARSE_MAX_TERMS)
        return false;
    g.L = sparse_list_L(k);
    const size_t per_query = sparse_image_bytes(n_vocab) + (size_t)g.L * 8 + 4;
    const int aim = qb_pref >= 1 && qb_pref <= SPARSE_QB_MAX ? qb_pref : SPARSE_QB[dtype];
    g.qb = (int)std::min<size_t>((size_t)std::min(aim, nq), SPARSE_LDS_MAX / per_query);
    if (g.qb < 1) return false;
    g.n_qtiles = (nq + g.qb - 1) / g.qb;
    const int s = std::max(1, std::min((TARGET_BLOCKS + g.n_qtiles - 1) / g.n_qtiles, n_rows / SPARSE_MIN_SLICE_ROWS));
    g.max_slices = s;
    const SliceCut c = slice_cut(n_rows, s, SPARSE_STEP_ROWS);
    g.slice_rows = c.rows; g.n_slices = c.n_slices;
    g.lds = (size_t)g.qb * per_query;
    return true;
}

// sparse_index_add_kernel: one workgroup per row.  Row first + i takes the entries of ids / weights [n][k_in] whose id is in
// [0, n_vocab), sorted by id (equal ids in input order), the weights rounded to the stored type; its other columns are zeroed.
struct SparseAddArgs {
    const int32_t *ids;
    const float *weights;
    void *sids, *sweights;              // the stored arrays
    int32_t *counts;
    int first, n, k_in, width, n_vocab;
};

// sparse_query_kernel: one workgroup per query, ids / weights [nq][kq] -> images [nq][img_bytes].  LDS: the image
struct SparseQueryArgs {
    const int32_t *ids;
    const float *weights;
    char *images;
    int nq, kq, n_vocab, words;
    unsigned img_bytes;
};

// sparse_index_scan_kernel.  LDS: as sparse_scan_geometry states
struct SparseScanArgs {
    const void *sids, *sweights;
    const int32_t *counts;
    const char *images;                 // [nq][img_bytes]
    float *ws_s;                        // [nq][n_slices][k] per-(query, slice) lists, best first
    int *ws_i;
    int n_rows, width, nq, qb, n_qtiles, n_slices, slice_rows, k, L, n_items, words;
    unsigned img_bytes;
    // words [ceil(n_rows / 32)], bit b of word w set = row 32 w + b is live / may be returned; either may be null = all ones (read by
    // the masked instantiation only, and last in the block: the unmasked one's argument offsets are what they were)
    const uint32_t *live, *allow;
    // the hybrid scan only (sparse_hybrid_scan_kernel, last in the block as live / allow were): the dense scores of the chunk's
    // queries, [nq][ld] with row r's at column r — read for qualifying rows alone —, and the two weights of
    // H = (w_dense * D) + (w_sparse * S)
    const float *dscores = nullptr;
    size_t ld = 0;
    float w_dense = 0.f, w_sparse = 0.f;
};

// Hybrid search (hybrid.cpp): the dense scores of one chunk of queries pass through HBM as a matrix [HC][ld], ld = n_rows rounded up
// to 64 floats.  HYBRID_SCORES_MAX bounds that workspace; it is a bound, not a tuned number.  hybrid_chunk_queries decides HC, the one
// place: the search and the test hook both call it.  HC is the most queries whose matrix fits the bound, at most nq and at most 4096
// (the chunk of both indexes), at least 1 — one query's scores are taken whatever they need —, and a multiple of 32 where it is
// 32 or more, so that the dense tiles stay full.  pref > 0 (the tuning key "hybrid_chunk_queries"): that chunk size instead, not
// rounded, under the same bounds.
constexpr size_t HYBRID_SCORES_MAX = (size_t)256 << 20;
inline size_t hybrid_ld(int n_rows) { return ((size_t)std::max(n_rows, 0) + 63) / 64 * 64; }
inline int hybrid_chunk_queries(int n_rows, int nq, int pref) {
    const size_t fit = HYBRID_SCORES_MAX / (std::max<size_t>(hybrid_ld(n_rows), 64) * 4);
    int hc = (int)std::min<size_t>(fit, (size_t)std::min(std::max(nq, 1), 4096));
    if (pref > 0) hc = std::min(hc, pref);
    else if (hc >= 32) hc = hc / 32 * 32;
    return std::max(hc, 1);
}

// sparse_index_rescore_kernel: one workgroup of SPARSE_RESCORE_CAND lanes per (query, chunk of its candidates); lane t scores row
// cand[q][chunk * SPARSE_RESCORE_CAND + t] against query q's image with the scan's chain and writes (score, id) — or (-inf, INT_MAX)
// for an id outside [0, n_rows) or a removed row — to ws [nq][n_cand], which topk_merge_kernel selects from.  LDS: one image
constexpr int SPARSE_RESCORE_CAND = 256;
constexpr int SPARSE_MAX_CAND = 1024;
struct SparseRescoreArgs {
    const void *sids, *sweights;
    const int32_t *counts;
    const char *images;                 // [nq][img_bytes]
    const uint32_t *live;               // null = every row live
    const int32_t *cand;                // [nq][n_cand]
    float *ws_s;                        // [nq][n_cand]
    int *ws_i;
    int n_rows, width, nq, n_cand, n_chunks, words;      // n_chunks = ceil(n_cand / SPARSE_RESCORE_CAND)
    unsigned img_bytes;
};

// sparse_index_gather_kernel (compaction): new row i < n of dst = the column slots in front of its count, and the count, of row
// old_ids[i] of src; every other slot of dst's ceil(n / 64) blocks — behind a count, or of a row at or beyond n — is zero
struct SparseGatherArgs {
    const void *sids, *sweights;
    const int32_t *counts, *old_ids;
    void *dids, *dweights;
    int32_t *dcounts;
    int n, width;
};

// sparse_index_export_kernel: out_ids / out_weights [n][width] = the stored rows rows[i]: ids ascending, then -1 with weight +0
struct SparseExportArgs {
    const void *sids, *sweights;
    const int32_t *counts, *rows;
    int32_t *out_ids;
    float *out_weights;
    int n, width;
};

// lets the scan kernels of the current device have SPARSE_LDS_MAX of LDS
void sparse_index_kernels_init();
void launch_sparse_add(int dtype, const SparseAddArgs &a, hipStream_t s);
void launch_sparse_query(const SparseQueryArgs &a, hipStream_t s);
// the masked instantiation iff a.live or a.allow is set
void launch_sparse_scan(int dtype, const SparseScanArgs &a, size_t lds, hipStream_t s);
// sparse_hybrid_scan_kernel: the scan with a.dscores, a.ld and the weights; masked iff a.live or a.allow is set
void launch_sparse_hybrid_scan(int dtype, const SparseScanArgs &a, size_t lds, hipStream_t s);
void launch_sparse_rescore(int dtype, const SparseRescoreArgs &a, hipStream_t s);
void launch_sparse_gather(int dtype, const SparseGatherArgs &a, hipStream_t s);
void launch_sparse_export(int dtype, const SparseExportArgs &a, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Postings and the inverted search (sparse_postings.hip; the class side is sparse_postings.cpp)
// ------------------------------------------------------------------------------------------------
// Postings: a second, term-major image of the stored rows.  The rows are cut into segments of seg rows (a multiple of
// SPARSE_STEP_ROWS, so a segment starts on a mask word; at most 16384, so a row number inside a segment is a u16).  Per segment a CSR
// over the vocabulary: off[segment][n_vocab + 1] u32, and two posting arrays as the rows have two — prow, the row number inside the
// segment (u16), and pw, the weight exactly as stored (f32 or f16).  Segment s owns the slots [s * seg * width, (s + 1) * seg * width)
// of both arrays (a segment never holds more terms); list id of segment s is slots s * seg * width + [off[s][id], off[s][id + 1]).
// The order of the entries inside a list is whatever the fill's atomics gave: every entry of a list belongs to another row.
constexpr int SPARSE_SEGMENT_ROWS = 2048;               // the default seg (the sweep it comes from)
constexpr int SPARSE_SEGMENT_ROWS_MAX = 16384;
constexpr int SPARSE_POSTINGS_QB = NWAVE;               // the most queries of a tile: one wave walks one query's lists
constexpr int SPARSE_POSTINGS_QB_AIM = 2;               // queries per tile the plan aims for: smaller tiles, more workgroups a CU
// "sparse_index_segment_rows": 256 .. 16384 in multiples of 256, anything else (0 included) = the default
inline int sparse_segment_rows(int pref) {
    return pref >= SPARSE_STEP_ROWS && pref <= SPARSE_SEGMENT_ROWS_MAX && pref % SPARSE_STEP_ROWS == 0 ? pref : SPARSE_SEGMENT_ROWS;
}
inline int sparse_segments(int n_rows, int seg) { return (int)(((long long)n_rows + seg - 1) / seg); }

// How a chunk of nq queries over n_rows rows in segments of seg rows is cut into workgroups of sparse_postings_scan_kernel: tiles of
// qb queries times slices of slice_segs whole segments, and a workgroup's LDS — per query seg f32 accumulators, its sorted terms
// (SPARSE_MAX_TERMS i32 ids and f32 weights) and a list of L = sparse_list_L(k) (score, id) entries, then a term count and a queue
// count per query.  The one place this is decided: the search and the test hook both call it.  qb_pref as sparse_scan_geometry's:
// 0, or the tile to aim for in place of SPARSE_POSTINGS_QB_AIM (values beyond SPARSE_POSTINGS_QB aim for that).  max_slices: what n_slices never exceeds and what never falls as n_rows grows.
struct SparsePostingsGeometry { int qb, n_qtiles, n_slices, slice_segs, L, max_slices, seg; size_t lds; };
inline bool sparse_postings_geometry(int dtype, int n_vocab, int n_rows, int nq, int k, int seg, SparsePostingsGeometry &g, int qb_pref = 0) {
    g = SparsePostingsGeometry{0, 0, 0, 0, 0, 0, 0, 0};
    if (dtype < 0 || dtype > 1 || n_vocab < 1 || n_vocab > SPARSE_MAX_VOCAB || (dtype == 1 && n_vocab > 65536) || n_rows < 0 || nq < 1 ||
        k < 1 || k > SPARSE_MAX_TERMS || seg < SPARSE_STEP_ROWS || seg > SPARSE_SEGMENT_ROWS_MAX || seg % SPARSE_STEP_ROWS != 0)
        return false;
    g.seg = seg;
    g.L = sparse_list_L(k);
    const size_t per_query = (size_t)seg * 4 + (size_t)SPARSE_MAX_TERMS * 8 + (size_t)g.L * 8 + 8;
    const int aim = qb_pref >= 1 ? std::min(qb_pref, SPARSE_POSTINGS_QB) : SPARSE_POSTINGS_QB_AIM;
    g.qb = (int)std::min<size_t>((size_t)std::min(aim, nq), SPARSE_LDS_MAX / per_query);
    if (g.qb < 1) return false;
    g.n_qtiles = (nq + g.qb - 1) / g.qb;
    const int n_segs = sparse_segments(n_rows, seg);
    const int s = std::max(1, std::min((TARGET_BLOCKS + g.n_qtiles - 1) / g.n_qtiles, n_segs));
    g.max_slices = s;
    g.slice_segs = std::max(1, (n_segs + s - 1) / s);
    g.n_slices = std::max(1, (n_segs + g.slice_segs - 1) / g.slice_segs);
    g.lds = (size_t)g.qb * per_query;
    return true;
}

// The three build kernels.  count: one thread per stored term of rows [0, n_rows), off[segment][id] += 1 (off zeroed before).
// scan: one workgroup per segment, off[segment][0 .. n_vocab] becomes the exclusive prefix sum in place (off[segment][n_vocab] the
// segment's term total).  fill: one thread per stored term, its place taken from cur — a copy of off that the fill consumes.
struct SparsePostingsBuildArgs {
    const void *sids, *sweights;        // the stored rows
    const int32_t *counts;
    uint32_t *off, *cur;                // [n_segs][n_vocab + 1]
    uint16_t *prow;
    void *pw;
    int n_rows, width, n_vocab, seg;
};

// sparse_query_sort_kernel: one workgroup per query, ids / weights [nq][kq] -> the query's terms with an id in [0, n_vocab) in
// ascending id (equal ids in input order), the weights as they are: tids / tw [nq][SPARSE_MAX_TERMS] and tn [nq]
struct SparseQuerySortArgs {
    const int32_t *ids;
    const float *weights;
    int32_t *tids;
    float *tw;
    int32_t *tn;
    int nq, kq, n_vocab;
};

// sparse_postings_scan_kernel.  LDS: as sparse_postings_geometry states
struct SparsePostingsScanArgs {
    const uint32_t *off;
    const uint16_t *prow;
    const void *pw;
    const int32_t *tids;                // the chunk's sorted queries (SparseQuerySortArgs)
    const float *tw;
    const int32_t *tn;
    float *ws_s;                        // [nq][n_slices][k] per-(query, slice) lists, best first
    int *ws_i;
    int n_rows, width, n_vocab, seg, nq, qb, n_qtiles, n_slices, slice_segs, k, L, n_items;
    const uint32_t *live, *allow;       // as SparseScanArgs's: read by the masked instantiation only
    // the hybrid scan only (sparse_postings_hybrid_scan_kernel), as SparseScanArgs's and last in the block as there: the dense scores
    // of the chunk's queries, [nq][ld] with GLOBAL row r's at column r — read for qualifying rows alone —, and the two weights
    const float *dscores = nullptr;
    size_t ld = 0;
    float w_dense = 0.f, w_sparse = 0.f;
};

// lets the postings scans of the current device have SPARSE_LDS_MAX of LDS
void sparse_postings_kernels_init();
// count, scan and fill of all segments of a.n_rows rows, in that order on s; a.off zeroed and a.cur = a.off copied in between
void launch_sparse_postings_build(int dtype, const SparsePostingsBuildArgs &a, hipStream_t s);
void launch_sparse_query_sort(const SparseQuerySortArgs &a, hipStream_t s);
// the masked instantiation iff a.live or a.allow is set
void launch_sparse_postings_scan(int dtype, const SparsePostingsScanArgs &a, size_t lds, hipStream_t s);
// sparse_postings_hybrid_scan_kernel: the same plan and LDS, selecting by hybrid_score(a.dscores, accumulator); masked iff a.live or
// a.allow is set
void launch_sparse_postings_hybrid_scan(int dtype, const SparsePostingsScanArgs &a, size_t lds, hipStream_t s);

}  // namespace bert_hip
