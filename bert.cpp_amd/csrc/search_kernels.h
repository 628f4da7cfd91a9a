// search_kernels.h — the device code of the embedding index (search.hip) as its host side (index.cpp) sees it: the argument
// blocks, the tile constants a search is planned with, and one launcher per kernel.  dtype is the index's: 0 f32, 1 f16, 2 i8,
// 3 b1 (search.hip states the forms).  A launcher only enqueues: the caller reads hipGetLastError.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "live_bits.h"

namespace bert_hip {

constexpr int QT = 32;                  // queries per workgroup tile: the M side of one 32 x 32 MFMA block
constexpr int NWAVE = 4;
constexpr int NT = 64 * NWAVE;
constexpr int STEP_ROWS = 32 * NWAVE;   // rows a workgroup scores per step (each wave one 32-row block)
constexpr int TARGET_BLOCKS = 2048;     // score workgroups a search aims for (8 per CU)

// The slice cut: n rows in s near-equal slices of whole steps (at least one): the rows of a slice, and how many slices that makes
struct SliceCut { int rows, n_slices; };
inline SliceCut slice_cut(int n, int s, int step) {
    const int per = (int)(((long long)n + s - 1) / s);
    const int rows = std::max(step, (per + step - 1) / step * step);
    return {rows, std::max(1, (int)(((long long)n + rows - 1) / rows))};
}

// index_topk_kernel.  LDS (lds bytes of launch_topk): float scores [min(QT, nq)][L], int ids the same, int count [QT]; L = index_topk_L(k)
inline int index_topk_L(int k) { return k + STEP_ROWS <= 256 ? 256 : 512; }
struct TopkArgs {
    const void *rows, *queries;          // [n_rows][dpad], [nq][dpad] of T (b1: rows of dpad bits, queries of dpad i8 codes)
    float *ws_s;                         // [nq][n_slices][k] per-(query, slice) lists, best first
    int *ws_i;
    int n_rows, dpad, nq, n_qtiles, n_slices, slice_rows, k, L, n_items;
    const float *qscale, *rscale;        // [nq], [n_rows]: i8 both, b1 qscale; null (never read) where the form has none
    // words [ceil(n_rows / 32)], bit b of word w set = row 32 w + b is live / may be returned; either may be null = all ones
    const uint32_t *live, *allow;
};

struct MergeArgs {
    const float *ws_s;                   // [nq][n_cand]
    const int *ws_i;
    int n_cand, k, L;                    // L = merge_L(k)
    int32_t *ids;                        // [nq][k]
    float *scores;
};
inline int merge_L(int k) { return k + NT <= 256 ? 256 : 512; }

struct RescoreArgs {
    const void *rows, *queries;          // as TopkArgs
    const float *qscale, *rscale;
    const uint32_t *live;                // null = every row live
    const int32_t *cand;                 // [nq][n_cand] ids; outside [0, n_rows) = no candidate
    float *ws_s;                         // [nq][n_cand]
    int *ws_i;
    int n_rows, dpad, nq, n_cand, n_blocks;      // n_blocks = ceil(n_cand / 32)
};

// index_scores_kernel (hybrid search): index_topk_kernel's scores without its selection, out[(q) * ld + row] for every query q of
// the chunk and every row whose bit of mask is set (mask null: every row); the other places of out are not written.  No LDS
struct ScoresArgs {
    const void *rows, *queries;          // as TopkArgs
    const float *qscale, *rscale;
    const uint32_t *mask;                // words [ceil(n_rows / 32)], bit set = the row's scores are wanted; null = all ones
    float *out;                          // [nq][ld]
    size_t ld;                           // floats per query of out, >= n_rows
    int n_rows, dpad, nq, n_qtiles, n_slices, slice_rows, n_items;
};
// How a chunk of nq queries over n_rows rows is cut into workgroups of index_scores_kernel: tiles of QT queries times slices of
// slice_rows rows (a multiple of STEP_ROWS), TARGET_BLOCKS workgroups aimed for, no slice shorter than 2048 rows
inline void index_scores_plan(int n_rows, int nq, ScoresArgs &a) {
    a.n_rows = n_rows; a.nq = nq;
    a.n_qtiles = (nq + QT - 1) / QT;
    const int s = std::max(1, std::min((TARGET_BLOCKS + a.n_qtiles - 1) / a.n_qtiles, n_rows / 2048));
    const SliceCut c = slice_cut(n_rows, s, STEP_ROWS);
    a.slice_rows = c.rows; a.n_slices = c.n_slices;
    a.n_items = a.n_qtiles * a.n_slices;
}

// index_probe_kernel: one workgroup per (query, item).  Items 0 .. nprobe - 1 are the lists probe[q][item] names (-1: none), whose
// members are order[offsets[l] .. offsets[l + 1]); item nprobe + c is tail chunk c, rows n_part + c * PROBE_CHUNK ... (< n_rows).
// LDS: float scores [L], int ids [L], int count, L = probe_L(k)
constexpr int PROBE_CHUNK = 1024;       // rows of a tail chunk
struct ProbeArgs {
    const void *rows, *queries;          // as TopkArgs
    const float *qscale, *rscale;
    const uint32_t *live;                // null = every row live
    const int32_t *probe;                // [nq][nprobe] list ids
    const int32_t *offsets, *order;      // [n_lists + 1], [offsets[n_lists]]
    float *ws_s;                         // [nq][n_items][k], best first
    int *ws_i;
    int n_rows, dpad, nq, nprobe, n_lists, n_part, n_items, k, L;
    // words shaped like live, bit set = the row may be returned; null = every row (read by the masked instantiation only, and
    // last in the block: the unmasked one's argument offsets are what they were)
    const uint32_t *allow;
};
inline int probe_L(int k) { return k + STEP_ROWS <= 256 ? 256 : 512; }

// index_export_kernel: out [n][dim] f32 = the stored rows ids[i] (ids null: first + i), as bert_hip_index_get_rows states them
struct ExportArgs {
    const void *rows;
    const float *rscale;
    const int32_t *ids;
    float *out;
    int first, n, dim, dpad;
};

// kmeans_update_kernel: one workgroup per list; centroid l := the sum of the exported rows order[offsets[l] .. offsets[l + 1])
// over its L2 norm, left as it is for an empty list or a zero or non-finite norm.  LDS: NWAVE * dim + NT floats
struct KmeansArgs {
    const void *rows;
    const float *rscale;
    const int32_t *offsets, *order;
    float *centroids;                    // [n_lists][dim]
    int n_lists, dim, dpad;
};

// lets every index_topk_kernel instantiation of the current device have the LDS of 32 queries x 512-entry lists
void search_kernels_init();
// the masked instantiation if a.live or a.allow is set
void launch_topk(int dtype, const TopkArgs &a, size_t lds, hipStream_t s);
void launch_topk_merge(const MergeArgs &a, int nq, hipStream_t s);
void launch_rescore(int dtype, const RescoreArgs &a, hipStream_t s);
// the masked instantiation iff a.mask is set
void launch_index_scores(int dtype, const ScoresArgs &a, hipStream_t s);
// out[w] = a[w] & b[w] & c[w] for w < n_words, a null pointer counting as all ones
void launch_mask_and(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, int n_words, hipStream_t s);
// the masked instantiation iff a.allow is set (removed rows alone stay on the unmasked one, which reads a.live per lane)
void launch_probe(int dtype, const ProbeArgs &a, hipStream_t s);
void launch_export(int dtype, const ExportArgs &a, hipStream_t s);
void launch_kmeans_update(int dtype, const KmeansArgs &a, hipStream_t s);
// f32 rows [n][dim] -> the stored form of dtype, [n][dpad] (scales [n]: i8 only)
void launch_ingest(int dtype, const float *src, void *dst, float *scales, int n, int dim, int dpad, hipStream_t s);
// row i of dst (row_bytes, a multiple of 16) = row old_ids[i] of src, and its scale with it (sscale null: the form has none)
void launch_gather(const void *src, void *dst, const float *sscale, float *dscale, const int32_t *old_ids, int n, size_t row_bytes, hipStream_t s);
// live bits of rows [first, first + n) := 1
void launch_live_set_range(uint32_t *live, int first, int n, hipStream_t s);
// (the same on a host mirror of the words, and the words that n rows take: live_set_range_host and live_words of live_bits.h)

}  // namespace bert_hip
