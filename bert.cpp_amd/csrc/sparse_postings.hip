// sparse_postings.hip — the device code of the sparse index's term-major form: the postings built from the stored rows and the
// inverted exact top-k search over them.  The layout, the plan and the argument blocks are in sparse_index_kernels.h ("Postings and
// the inverted search"); the class side is sparse_postings.cpp.
//
//   sparse_postings_count_kernel<DTYPE> / _offsets_kernel / _fill_kernel<DTYPE>   the build: the number of stored terms per (segment, id) with
//                         integer atomics, an exclusive prefix sum per segment in place, and the fill — every stored term takes the
//                         next free slot of its list from a copy of the offsets and writes its row number inside the segment and its
//                         weight as stored.  The order inside a list is the atomics' and differs from build to build.
//   sparse_query_sort_kernel   one workgroup per query: rank-by-count (sparse_device.h) turns the query into its terms in ascending id,
//                         ids in [0, n_vocab), weights unrounded, and a count.
//   sparse_postings_scan_kernel<DTYPE, MASKED>   one workgroup of four waves per (slice of whole segments, tile of qb <= 4 queries, 2 unless asked otherwise).
//                         LDS holds per query seg f32 accumulators, the sorted terms and the scan's list.  Per segment: all lanes zero
//                         the accumulators; wave q walks query q's terms alone, in ascending id — the offsets of 64 terms are loaded
//                         together, one per lane, then term after term the wave reads that list coalesced and runs
//                         acc[row] = fmaf(w, qw, acc[row]) in LDS —; then all lanes walk the segment's rows, 256 per step, and select
//                         with topk_select.h's queue: one list per query of the tile, a threshold pair per query in registers.
//   sparse_postings_hybrid_scan_kernel<DTYPE, MASKED>   the same body as the second pass of a hybrid search over the postings
//                         (hybrid.cpp): a row is selected by hybrid_score(D, accumulator), D read from the matrix index_scores_kernel
//                         (search.hip) wrote, at [query inside the chunk][global row], a step ahead of its use.
//
// The one rule: all updates of one accumulator happen in ascending term id, so a row's chain is the score rule of bert_hip.h and its
// bits are the row-major search's.  Inside one list every entry is another row, so the lanes of one instruction, and the passes over
// one list, never meet on an accumulator; between two terms the walking wave waits for its LDS operations (s_waitcnt lgkmcnt(0), which
// also keeps the compiler from moving a term's reads above the previous term's writes).  No other wave touches that query's
// accumulators between the two barriers around the walk.
//
// Bounds: a sorted term's id is in [0, n_vocab), so off[id] and off[id + 1] exist; a list lies inside its segment's seg * width slots
// (a segment holds at most that many terms); a posting's row number is below seg by construction; a row at or beyond n_rows is never
// selected and no mask word at or beyond ceil(n_rows / 32) is read.
#include <hip/hip_runtime.h>

#include <cmath>

#include "device.h"
#include "hybrid_score.h"
#include "sparse_device.h"
#include "topk_select.h"

namespace bert_hip {

namespace {

constexpr int QB_MAX = SPARSE_POSTINGS_QB;

// Both passes over the stored rows visit the slots of the blocks in storage order (slot_decode)
template <int DTYPE>
__global__ __launch_bounds__(256) void sparse_postings_count_kernel(SparsePostingsBuildArgs a) {
    using id_t = typename Stored<DTYPE>::id_t;
    const size_t total = block_slots(a.n_rows, a.width);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        int row, j;
        slot_decode(e, a.width, row, j);
        if (row >= a.n_rows || j >= a.counts[row]) continue;
        const int id = (int)((const id_t *)a.sids)[e];
        if (id < 0 || id >= a.n_vocab) continue;               // (never stored: add and load see to it)
        atomicAdd(&a.off[(size_t)(row / a.seg) * (a.n_vocab + 1) + id], 1u);
    }
}

// one workgroup per segment: thread t owns entries [t * chunk, (t + 1) * chunk) of the segment's n_vocab + 1
__global__ __launch_bounds__(256) void sparse_postings_offsets_kernel(SparsePostingsBuildArgs a) {
    __shared__ uint32_t part[256];
    const int t = threadIdx.x, n = a.n_vocab + 1;
    uint32_t *off = a.off + (size_t)blockIdx.x * n;
    const int chunk = (n + 255) / 256, x0 = min(n, t * chunk), x1 = min(n, x0 + chunk);
    uint32_t sum = 0;
    for (int x = x0; x < x1; ++x) sum += off[x];
    part[t] = sum;
    __syncthreads();
    uint32_t below = 0;
    for (int u = 0; u < t; ++u) below += part[u];
    for (int x = x0; x < x1; ++x) { const uint32_t c = off[x]; off[x] = below; below += c; }
}

template <int DTYPE>
__global__ __launch_bounds__(256) void sparse_postings_fill_kernel(SparsePostingsBuildArgs a) {
    using id_t = typename Stored<DTYPE>::id_t;
    using w_t = typename Stored<DTYPE>::w_t;
    const size_t per_seg = (size_t)a.seg * a.width, total = block_slots(a.n_rows, a.width);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        int row, j;
        slot_decode(e, a.width, row, j);
        if (row >= a.n_rows || j >= a.counts[row]) continue;
        const int id = (int)((const id_t *)a.sids)[e];
        if (id < 0 || id >= a.n_vocab) continue;
        const int sg = row / a.seg;
        const uint32_t p = atomicAdd(&a.cur[(size_t)sg * (a.n_vocab + 1) + id], 1u);
        if (p >= per_seg) continue;                            // (cannot happen: the count pass saw the same terms)
        a.prow[(size_t)sg * per_seg + p] = (uint16_t)(row - sg * a.seg);
        ((w_t *)a.pw)[(size_t)sg * per_seg + p] = ((const w_t *)a.sweights)[e];
    }
}

__global__ __launch_bounds__(256) void sparse_query_sort_kernel(SparseQuerySortArgs a) {
    __shared__ int keys[SPARSE_MAX_TERMS];
    const int t = threadIdx.x, q = blockIdx.x;
    const RankedTerm r = rank_terms(a.ids, a.weights, (size_t)q * a.kq, a.kq, a.n_vocab, keys, t);
    // (count <= kq <= 256; the places behind count are never read)
    if (r.key != INT_MAX) {
        a.tids[(size_t)q * SPARSE_MAX_TERMS + r.rank] = r.key;
        a.tw[(size_t)q * SPARSE_MAX_TERMS + r.rank] = r.w;
    }
    if (t == 0) a.tn[q] = r.count;
}

// When the hybrid scan asks for a step's dense scores: 1 = one step ahead — the first step's before the segment's term walk, each
// later step's at the top of the step before it —, 0 = at the top of the step that uses them (the A/B of DESIGN.md §15.1)
#ifndef SPARSE_POSTINGS_D_AHEAD
#define SPARSE_POSTINGS_D_AHEAD 1
#endif

// The scan's body, shared by sparse_postings_scan_kernel and sparse_postings_hybrid_scan_kernel.
// HYBRID (the second pass of a hybrid search over the postings, hybrid.cpp): in the row walk a lane whose row qualifies holds its
// row's dense score of each query of the tile, read from a.dscores at [query inside the chunk][GLOBAL row] (lane = row: one coalesced
// 1 KiB access per query and step), and the score the row is selected by is hybrid_score(D, accumulator) in place of the
// accumulator.  A lane whose row does not qualify, or lies at or beyond n_rows, reads nothing — the dense pass may not have written
// there.  The loads are issued a step ahead, into registers: the first step's before the term walk, whose length hides them (and
// which the waves without a query of their own only wait for), each later step's at the top of the step before it, so that no
// step waits for the HBM.  No LDS beyond the plain scan's: sparse_postings_geometry is the plan of both.
template <int DTYPE, bool MASKED, bool HYBRID>
__device__ __forceinline__ void sparse_postings_scan_body(const SparsePostingsScanArgs &a) {
    using w_t = typename Stored<DTYPE>::w_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int item = xcd_item();                 // (kernels.h: the query tiles of one slice go to one XCD and find its postings in that L2)
    if (item >= a.n_items) return;
    const int slice = item / a.n_qtiles, qt = item - slice * a.n_qtiles;
    const int q0 = qt * a.qb, nqv = min(a.qb, a.nq - q0);
    const int seg = a.seg, L = a.L, k = a.k;
    const int n_segs = (int)(((long long)a.n_rows + seg - 1) / seg);
    const int s0 = slice * a.slice_segs, s1 = min(n_segs, s0 + a.slice_segs);
    float *acc = (float *)smem;                                // [qb][seg]
    int *tids = (int *)(acc + (size_t)a.qb * seg);             // [qb][SPARSE_MAX_TERMS]
    float *tw = (float *)(tids + a.qb * SPARSE_MAX_TERMS);
    float *ls = tw + a.qb * SPARSE_MAX_TERMS;                  // [qb][L]
    int *li = (int *)(ls + a.qb * L);
    int *tn = li + a.qb * L;                                   // [qb], the counts [qb] behind
    // a step pushes at most SPARSE_STEP_ROWS entries per query
    const SelectLists sel{ls, li, tn + a.qb, L, k, L - k - SPARSE_STEP_ROWS};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    select_init(sel, nqv, tid);
    if (tid < nqv) tn[tid] = min(max(a.tn[q0 + tid], 0), SPARSE_MAX_TERMS);
    __syncthreads();
    // (only the terms in front of a query's count were written by the sort)
    for (int i = tid; i < nqv * SPARSE_MAX_TERMS; i += NT) {
        const bool in = (i & (SPARSE_MAX_TERMS - 1)) < tn[i / SPARSE_MAX_TERMS];
        tids[i] = in ? a.tids[(size_t)q0 * SPARSE_MAX_TERMS + i] : 0;
        tw[i] = in ? a.tw[(size_t)q0 * SPARSE_MAX_TERMS + i] : 0.f;
    }
    float ts[QB_MAX];
    int ti[QB_MAX];
#pragma unroll
    for (int q = 0; q < QB_MAX; ++q) { ts[q] = -INFINITY; ti[q] = SENT_ID; }
    __syncthreads();

    // does row r0 + lrow of a segment of nrow rows qualify (lrow < seg: a step never leaves the segment)
    auto qualifies = [&](int lrow, int row, int nrow) -> bool {
        bool ok = lrow < nrow;
        if constexpr (MASKED) {
            if (ok) {
                uint32_t m = ~0u;
                if (a.live) m &= a.live[row >> 5];
                if (a.allow) m &= a.allow[row >> 5];
                ok = (m >> (row & 31)) & 1u;
            }
        }
        return ok;
    };
    // HYBRID: the dense scores of a qualifying row, one per query of the tile.  One branch around all of them and none between them —
    // a place behind the tile's last query reads that query's score again (inside the matrix, and never used) —, so that the loads
    // go out together: behind a branch of its own each load would be waited for before the next is issued
    auto load_dense = [&](bool ok, int row, float (&d)[QB_MAX]) {
#pragma unroll
        for (int q = 0; q < QB_MAX; ++q) d[q] = 0.f;
        if (ok) {
            const float *p = a.dscores + (size_t)q0 * a.ld + row;
#pragma unroll
            for (int q = 0; q < QB_MAX; ++q) d[q] = p[(size_t)min(q, nqv - 1) * a.ld];
        }
    };
    for (int sg = s0; sg < s1; ++sg) {
        const int r0 = sg * seg, nrow = min(seg, a.n_rows - r0);
        // HYBRID: the first step's row state and dense scores, asked for ahead of the walk
        [[maybe_unused]] float dv[QB_MAX];
        [[maybe_unused]] bool dok = false;
        if constexpr (HYBRID && SPARSE_POSTINGS_D_AHEAD) {
            dok = qualifies(tid, r0 + tid, nrow);
            load_dense(dok, r0 + tid, dv);
        }
        // 1. zero the accumulators (the barrier that ends the previous segment's last step stands in front)
        for (int i = tid * 4; i < nqv * seg; i += NT * 4) *(f32x4 *)(acc + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        // 2. wave q walks query q's terms in ascending id
        if (wave < nqv) {
            const int nt = __builtin_amdgcn_readfirstlane(tn[wave]);
            const uint32_t *off = a.off + (size_t)sg * (a.n_vocab + 1);
            const size_t pbase = (size_t)sg * seg * a.width;
            const uint16_t *pr = a.prow + pbase;
            const w_t *pw = (const w_t *)a.pw + pbase;
            const uint32_t pmax = (uint32_t)seg * (uint32_t)a.width;
            float *ac = acc + wave * seg;
            for (int t0 = 0; t0 < nt; t0 += 64) {
                // the offsets of up to 64 terms, one term per lane: independent loads, issued together
                uint32_t b = 0, e = 0;
                float qw = 0.f;
                if (t0 + lane < nt) {
                    const int id = tids[wave * SPARSE_MAX_TERMS + t0 + lane];
                    b = off[id];
                    e = min(off[id + 1], pmax);
                    qw = tw[wave * SPARSE_MAX_TERMS + t0 + lane];
                }
                const int nu = min(64, nt - t0);
                for (int u = 0; u < nu; ++u) {
                    const uint32_t bu = (uint32_t)__builtin_amdgcn_readlane((int)b, u), eu = (uint32_t)__builtin_amdgcn_readlane((int)e, u);
                    const float wu = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qw), u));
                    for (uint32_t p = bu + lane; p < eu; p += 64) {
                        const int lr = min((int)pr[p], seg - 1);
                        const float w = (float)pw[p];
                        ac[lr] = __builtin_fmaf(w, wu, ac[lr]);
                    }
                    // the next term's reads follow this term's writes, in the program and in the LDS
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            }
        }
        __syncthreads();
        // 3. all lanes walk the segment's rows
        for (int b0 = 0; b0 < nrow; b0 += SPARSE_STEP_ROWS) {
            const int lrow = b0 + tid, row = r0 + lrow;        // (lrow < seg: b0 and seg are multiples of the step)
            bool rok;
            [[maybe_unused]] float dn[QB_MAX];
            [[maybe_unused]] bool nok = false;
            if constexpr (HYBRID && SPARSE_POSTINGS_D_AHEAD) {
                rok = dok;
                // the next step's, before this step's selection (a step behind the segment's last has no rows: nothing is asked for)
                nok = b0 + SPARSE_STEP_ROWS < nrow && qualifies(lrow + SPARSE_STEP_ROWS, row + SPARSE_STEP_ROWS, nrow);
                load_dense(nok, row + SPARSE_STEP_ROWS, dn);
            } else {
                rok = qualifies(lrow, row, nrow);
                if constexpr (HYBRID) load_dense(rok, row, dv);
            }
#pragma unroll
            for (int q = 0; q < QB_MAX; ++q)
                if (q < nqv) {
                    float s = acc[q * seg + lrow];
                    if constexpr (HYBRID) s = hybrid_score(a.w_dense, dv[q], a.w_sparse, s);
                    if (rok && better(s, row, ts[q], ti[q])) select_push(sel, q, s, row);
                }
            if (select_step_end(sel, nqv, tid)) {
#pragma unroll
                for (int q = 0; q < QB_MAX; ++q)
                    if (q < nqv) select_threshold(sel, q, ts[q], ti[q]);
                select_resume(sel, nqv, tid);
            }
            if constexpr (HYBRID && SPARSE_POSTINGS_D_AHEAD) {
                dok = nok;
#pragma unroll
                for (int q = 0; q < QB_MAX; ++q) dv[q] = dn[q];
            }
        }
    }
    select_finish(sel, nqv, tid);
    select_store(sel, nqv, a.ws_s, a.ws_i, q0, a.n_slices, slice, tid);
}

template <int DTYPE, bool MASKED>
__global__ __launch_bounds__(NT) void sparse_postings_scan_kernel(SparsePostingsScanArgs a) { sparse_postings_scan_body<DTYPE, MASKED, false>(a); }

template <int DTYPE, bool MASKED>
__global__ __launch_bounds__(NT) void sparse_postings_hybrid_scan_kernel(SparsePostingsScanArgs a) { sparse_postings_scan_body<DTYPE, MASKED, true>(a); }

DeviceFlags g_postings_lds;

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers (sparse_index_kernels.h)
// ------------------------------------------------------------------------------------------------
void sparse_postings_kernels_init() {
    scan_lds_opt_in(g_postings_lds, {SPARSE_SCAN_FAMILY(sparse_postings_scan_kernel), SPARSE_SCAN_FAMILY(sparse_postings_hybrid_scan_kernel)});
}

void launch_sparse_postings_build(int dtype, const SparsePostingsBuildArgs &a, hipStream_t s) {
    if (a.n_rows <= 0) return;
    const int n_segs = sparse_segments(a.n_rows, a.seg);
    const size_t off_bytes = (size_t)n_segs * (a.n_vocab + 1) * 4;
    const int blocks = (int)std::min<size_t>((block_slots(a.n_rows, a.width) + 255) / 256, 16384);
    (void)hipMemsetAsync(a.off, 0, off_bytes, s);
    if (dtype == 1) BERT_LAUNCH(sparse_postings_count_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
    else BERT_LAUNCH(sparse_postings_count_kernel<0>, dim3(blocks), dim3(256), 0, s, a);
    BERT_LAUNCH(sparse_postings_offsets_kernel, dim3((unsigned)n_segs), dim3(256), 0, s, a);
    (void)hipMemcpyAsync(a.cur, a.off, off_bytes, hipMemcpyDeviceToDevice, s);
    if (dtype == 1) BERT_LAUNCH(sparse_postings_fill_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
    else BERT_LAUNCH(sparse_postings_fill_kernel<0>, dim3(blocks), dim3(256), 0, s, a);
}

void launch_sparse_query_sort(const SparseQuerySortArgs &a, hipStream_t s) {
    BERT_LAUNCH(sparse_query_sort_kernel, dim3((unsigned)a.nq), dim3(256), 0, s, a);
}

void launch_sparse_postings_scan(int dtype, const SparsePostingsScanArgs &a, size_t lds, hipStream_t s) {
    SPARSE_SCAN_LAUNCH(sparse_postings_scan_kernel, dtype, a, lds, s);
}

void launch_sparse_postings_hybrid_scan(int dtype, const SparsePostingsScanArgs &a, size_t lds, hipStream_t s) {
    SPARSE_SCAN_LAUNCH(sparse_postings_hybrid_scan_kernel, dtype, a, lds, s);
}

}  // namespace bert_hip
