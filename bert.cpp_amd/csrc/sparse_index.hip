// sparse_index.hip — the device code of the sparse index: rows of (vocabulary id, weight) terms in HBM and their exact top-k
// inner-product search.  The kernels and their launchers (sparse_index_kernels.h, which states the stored form and the query image);
// the SparseIndex class that plans and orders them is sparse_index.cpp (sparse_index.h).
//
//   sparse_index_add_kernel<DTYPE>   one workgroup per row: drops the entries whose id is outside [0, n_vocab), ranks the others by id
//                         (rank_terms, sparse_device.h: a count over the row's keys in LDS; equal ids keep their input order), rounds the weights to the
//                         stored type and writes the row's column slots in its block of 64, zeros behind its terms, and its count.  A
//                         row's place depends on its id alone, so an add may start and end anywhere inside a block.
//   sparse_query_kernel   one workgroup per query: sets the bitmap's bits with LDS atomics, scans the per-word counts, lets each term
//                         compute its own rank and store its weight there — no sort —, and writes the image to the chunk's buffer.
//   sparse_index_scan_kernel<DTYPE, MASKED>  one workgroup of four waves per (slice of row blocks, tile of qb queries).  It stages the tile's
//                         images in LDS; each wave walks one block per step, column by column: a lane loads its row's (id, w) of the
//                         column once and, for each query of the tile, tests the id's bit and on a hit runs
//                         acc[q] = fmaf(w, qw[prefix[id >> 5] + popc(word & below)], acc[q]).  The columns are in ascending id, so a
//                         lane's chain IS the score rule of bert_hip.h; there is no cross-lane reduction.  A block is walked to the
//                         largest count of its 64 rows (a wave maximum), not to width.  Selection is topk_select.h's protocol (written
//                         out in the body: see there), one list per query of the tile and a threshold pair per query in
//                         registers: one sorted list per (query, slice) into the workspace — which topk_merge_kernel merges.
//                         The MASKED instantiation (removed rows, an allow-list) reads two mask words per block: see the kernel.
//   sparse_hybrid_scan_kernel<DTYPE, MASKED>  the same body as the second pass of a hybrid search (hybrid.cpp): the score a row is
//                         selected by is (w_dense * D) + (w_sparse * S), D read from the matrix index_scores_kernel (search.hip) wrote.
//   sparse_index_rescore_kernel<DTYPE>  per-query candidate rows against that query's image, one row per lane, the scan's chain.
//   sparse_index_gather_kernel<DTYPE>   compaction: the live rows' columns and counts into a fresh allocation.
//   sparse_index_export_kernel<DTYPE>  stored rows, named by id, back as (i32 id, f32 weight) columns: bert_hip_sparse_index_get_rows.
//
// Bounds: every id that reaches storage or an image is in [0, n_vocab), whatever the caller's arrays hold, so the scan's LDS reads stay
// inside the image (word index < words, rank < 256: at most 256 bits are ever set); a lane whose row is past the rows, or whose column
// is past its count, reads nothing and uses id 0.
#include <hip/hip_runtime.h>

#include <cmath>

#include "device.h"
#include "hybrid_score.h"
#include "sparse_device.h"
#include "topk_select.h"

namespace bert_hip {

namespace {

constexpr int QB_MAX = SPARSE_QB_MAX;   // the most queries of a tile (registers: one accumulator and one threshold pair each)
constexpr int COL_U = 8;                // columns of a block whose loads are in flight together
static_assert(SPARSE_QB[0] <= QB_MAX && SPARSE_QB[1] <= QB_MAX, "a tile's accumulators are registers");

template <int DTYPE>
__global__ __launch_bounds__(256) void sparse_index_add_kernel(SparseAddArgs a) {
    using id_t = typename Stored<DTYPE>::id_t;
    using w_t = typename Stored<DTYPE>::w_t;
    __shared__ int keys[SPARSE_MAX_TERMS], skeys[SPARSE_MAX_TERMS];
    __shared__ float vals[SPARSE_MAX_TERMS];
    const int t = threadIdx.x, i = blockIdx.x, row = a.first + i;
    const RankedTerm r = rank_terms(a.ids, a.weights, (size_t)i * a.k_in, a.k_in, a.n_vocab, keys, t);
    // (count <= k_in <= width)
    if (r.key != INT_MAX) { skeys[r.rank] = r.key; vals[r.rank] = r.w; }
    __syncthreads();
    if (t < a.width) {
        const size_t o = slot(row, t, a.width);
        ((id_t *)a.sids)[o] = t < r.count ? (id_t)skeys[t] : (id_t)0;
        ((w_t *)a.sweights)[o] = t < r.count ? (w_t)vals[t] : (w_t)0.f;     // (f16: round to nearest even)
    }
    if (t == 0) a.counts[row] = r.count;
}

__global__ __launch_bounds__(256) void sparse_query_kernel(SparseQueryArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int part[256];
    const int t = threadIdx.x, q = blockIdx.x, words = a.words;
    uint32_t *bm = (uint32_t *)smem;
    uint16_t *pf = (uint16_t *)(smem + (size_t)words * 4);
    float *qw = (float *)(smem + (size_t)words * 4 + (((size_t)words * 2 + 3) & ~(size_t)3));
    for (unsigned i = t; i < a.img_bytes / 4; i += 256) ((uint32_t *)smem)[i] = 0u;
    __syncthreads();
    int id = -1;
    float w = 0.f;
    if (t < a.kq) {
        id = a.ids[(size_t)q * a.kq + t];
        if (id >= 0 && id < a.n_vocab) w = a.weights[(size_t)q * a.kq + t];
        else id = -1;
    }
    if (id >= 0) atomicOr(&bm[id >> 5], 1u << (id & 31));
    __syncthreads();
    // the set bits below each word: thread t owns words [w0, w1)
    const int chunk = (words + 255) / 256, w0 = min(words, t * chunk), w1 = min(words, w0 + chunk);
    int sum = 0;
    for (int x = w0; x < w1; ++x) sum += __popc(bm[x]);
    part[t] = sum;
    __syncthreads();
    int below = 0;
    for (int u = 0; u < t; ++u) below += part[u];
    for (int x = w0; x < w1; ++x) { pf[x] = (uint16_t)below; below += __popc(bm[x]); }
    __syncthreads();
    if (id >= 0) qw[pf[id >> 5] + __popc(bm[id >> 5] & ((1u << (id & 31)) - 1u))] = w;
    __syncthreads();
    u32x4 *dst = (u32x4 *)(a.images + (size_t)q * a.img_bytes);
    for (unsigned i = t; i < a.img_bytes / 16; i += 256) dst[i] = ((const u32x4 *)smem)[i];
}

// The scan's body, shared by sparse_index_scan_kernel and sparse_hybrid_scan_kernel.
// MASKED (removed rows or an allow-list): a row qualifies iff its bit of live & allow is set.  A wave's block of 64 rows starts at a
// multiple of 64 (slices start at multiples of SPARSE_STEP_ROWS), so its mask is two words, the same for all its lanes, loaded
// through the scalar path; a lane whose bit is clear is a lane past the rows — count 0, no push —, so a block is walked to the largest
// count of its qualifying rows and one without any issues no column load.  No word at or beyond ceil(n_rows / 32) is read.
//
// HYBRID (sparse_hybrid_scan_kernel, the second pass of a hybrid search): at the top of a step, before the column walk so that the
// loads' latency hides under it, a lane whose row qualifies loads its row's dense score of each query of the tile from a.dscores
// (lane = row: a coalesced 256-byte access per query); a lane whose row does not qualify reads nothing — the dense pass may not
// have written there.  After the walk the score is hybrid_score(D, S) in place of S; everything behind it is the scan's.
//
// The selection is written out here, not taken from topk_select.h's helpers: with them this scan measured slower.
// The protocol and its barrier contract are the ones stated there.
template <int DTYPE, bool MASKED, bool HYBRID>
__device__ __forceinline__ void sparse_scan_body(const SparseScanArgs &a) {
    using id_t = typename Stored<DTYPE>::id_t;
    using w_t = typename Stored<DTYPE>::w_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int item = xcd_item();                 // (kernels.h: the query tiles of one slice of rows go to one XCD)
    if (item >= a.n_items) return;
    const int slice = item / a.n_qtiles, qt = item - slice * a.n_qtiles;
    const int q0 = qt * a.qb, nqv = min(a.qb, a.nq - q0);
    const int r0 = slice * a.slice_rows, r1 = min(a.n_rows, r0 + a.slice_rows);
    const int L = a.L, k = a.k, words = a.words;
    const unsigned img_bytes = a.img_bytes;
    float *ls = (float *)(smem + (size_t)a.qb * img_bytes);
    int *li = (int *)(ls + a.qb * L);
    int *cnt = li + a.qb * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pf_off = (size_t)words * 4, qw_off = pf_off + (((size_t)words * 2 + 3) & ~(size_t)3);

    {
        const u32x4 *src = (const u32x4 *)(a.images + (size_t)q0 * img_bytes);
        const unsigned n16 = (unsigned)nqv * (img_bytes / 16);
        for (unsigned i = tid; i < n16; i += NT) ((u32x4 *)smem)[i] = src[i];
    }
    for (int i = tid; i < nqv * L; i += NT) { ls[i] = -INFINITY; li[i] = SENT_ID; }
    if (tid < nqv) cnt[tid] = 0;
    float ts[QB_MAX];
    int ti[QB_MAX];
#pragma unroll
    for (int q = 0; q < QB_MAX; ++q) { ts[q] = -INFINITY; ti[q] = SENT_ID; }
    __syncthreads();

    // a step pushes at most SPARSE_STEP_ROWS entries per query: sort before a queue could hold fewer free slots
    const int room = L - k - SPARSE_STEP_ROWS;
    for (int base = r0; base < r1; base += SPARSE_STEP_ROWS) {
        const int brow = base + wave * SPARSE_BLOCK_ROWS, row = brow + lane;
        const bool inb = row < r1;
        bool rok = inb;
        if constexpr (MASKED) {
            const int blk = __builtin_amdgcn_readfirstlane(brow);
            uint32_t m0 = 0, m1 = 0;
            if (blk < r1) {                                    // (a block at or beyond r1 has no words)
                const int wi = blk >> 5;
                m0 = ~0u;
                if (a.live) m0 &= a.live[wi];
                if (a.allow) m0 &= a.allow[wi];
                if (blk + 32 < a.n_rows) {                     // (the second word exists: wi + 1 < ceil(n_rows / 32))
                    m1 = ~0u;
                    if (a.live) m1 &= a.live[wi + 1];
                    if (a.allow) m1 &= a.allow[wi + 1];
                }
            }
            m0 = __builtin_amdgcn_readfirstlane(m0);
            m1 = __builtin_amdgcn_readfirstlane(m1);
            rok = rok && (((lane < 32 ? m0 : m1) >> (lane & 31)) & 1u);
        }
        [[maybe_unused]] float dv[QB_MAX];
        if constexpr (HYBRID) {
#pragma unroll
            for (int q = 0; q < QB_MAX; ++q) dv[q] = q < nqv && rok ? a.dscores[(size_t)(q0 + q) * a.ld + row] : 0.f;
        }
        const int n = rok ? a.counts[row] : 0;
        int nmax = n;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o));
        nmax = min(__builtin_amdgcn_readfirstlane(nmax), a.width);
        float acc[QB_MAX];
#pragma unroll
        for (int q = 0; q < QB_MAX; ++q) acc[q] = 0.f;
        const id_t *ip = (const id_t *)a.sids + slot(inb ? row : r0, 0, a.width);
        const w_t *wp = (const w_t *)a.sweights + slot(inb ? row : r0, 0, a.width);
        // COL_U columns at a time: their loads are issued together — unconditional, as stored (no conversion between them, which
        // would wait for each), from a column the block has: what a lane reads past its count is masked below —, then the columns
        // are consumed in j order (the chain's order)
        for (int j0 = 0; j0 < nmax; j0 += COL_U) {
            id_t idv[COL_U];
            w_t wv[COL_U];
#pragma unroll
            for (int u = 0; u < COL_U; ++u) {
                const size_t o = (size_t)min(j0 + u, a.width - 1) * SPARSE_BLOCK_ROWS;
                idv[u] = ip[o];
                wv[u] = wp[o];
            }
#pragma unroll
            for (int u = 0; u < COL_U; ++u) {
                const bool act = j0 + u < n;
                const int id = act ? (int)idv[u] : 0;
                const float w = (float)wv[u];
                const int wi = id >> 5;
                const uint32_t bit = 1u << (id & 31);
#pragma unroll
                for (int q = 0; q < QB_MAX; ++q)
                    if (q < nqv) {
                        const char *img = smem + (size_t)q * img_bytes;
                        const uint32_t word = ((const uint32_t *)img)[wi];
                        if (act && (word & bit)) {
                            const int r = (int)((const uint16_t *)(img + pf_off))[wi] + __popc(word & (bit - 1u));
                            acc[q] = __builtin_fmaf(w, ((const float *)(img + qw_off))[r], acc[q]);
                        }
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < QB_MAX; ++q)
            if (q < nqv) {
                float s = acc[q];
                if constexpr (HYBRID) s = hybrid_score(a.w_dense, dv[q], a.w_sparse, acc[q]);
                if (rok && better(s, row, ts[q], ti[q])) {
                    const int p = atomicAdd(&cnt[q], 1);
                    ls[q * L + k + p] = s;
                    li[q * L + k + p] = row;
                }
            }
        __syncthreads();
        if (__syncthreads_or(tid < nqv && cnt[tid] > room)) {
            bitonic_sort_lists(ls, li, nqv, L, tid);
            if (tid < nqv) cnt[tid] = 0;
#pragma unroll
            for (int q = 0; q < QB_MAX; ++q)
                if (q < nqv) { ts[q] = ls[q * L + k - 1]; ti[q] = li[q * L + k - 1]; }
            __syncthreads();
        }
    }
    __syncthreads();
    if (__syncthreads_or(tid < nqv && cnt[tid] > 0)) bitonic_sort_lists(ls, li, nqv, L, tid);
    for (int i = tid; i < nqv * k; i += NT) {
        const int q = i / k, j = i - q * k;
        const size_t o = ((size_t)(q0 + q) * a.n_slices + slice) * k + j;
        a.ws_s[o] = ls[q * L + j];
        a.ws_i[o] = li[q * L + j];
    }
}

template <int DTYPE, bool MASKED>
__global__ __launch_bounds__(NT) void sparse_index_scan_kernel(SparseScanArgs a) { sparse_scan_body<DTYPE, MASKED, false>(a); }

template <int DTYPE, bool MASKED>
__global__ __launch_bounds__(NT) void sparse_hybrid_scan_kernel(SparseScanArgs a) { sparse_scan_body<DTYPE, MASKED, true>(a); }

template <int DTYPE>
__global__ __launch_bounds__(256) void sparse_index_export_kernel(SparseExportArgs a) {
    using id_t = typename Stored<DTYPE>::id_t;
    using w_t = typename Stored<DTYPE>::w_t;
    const size_t total = (size_t)a.n * a.width;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / a.width;
        const int j = (int)(e - i * a.width), row = a.rows[i];
        const bool in = j < a.counts[row];
        const size_t o = slot(row, j, a.width);
        a.out_ids[e] = in ? (int32_t)((const id_t *)a.sids)[o] : -1;
        a.out_weights[e] = in ? (float)((const w_t *)a.sweights)[o] : 0.f;
    }
}

// One workgroup per (query, chunk of SPARSE_RESCORE_CAND candidates).  It stages the query's image in LDS; lane t takes one candidate id
// and walks its own row's columns j < count in ascending j with the scan's expression from +0 — the score bits of a search.  The loads
// are strided (a row per lane), not coalesced: candidates are few.  The barrier stands in front of the per-lane walk.
template <int DTYPE>
__global__ __launch_bounds__(SPARSE_RESCORE_CAND) void sparse_index_rescore_kernel(SparseRescoreArgs a) {
    using id_t = typename Stored<DTYPE>::id_t;
    using w_t = typename Stored<DTYPE>::w_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const int q = (int)blockIdx.x / a.n_chunks, c = ((int)blockIdx.x - q * a.n_chunks) * SPARSE_RESCORE_CAND + t;
    {
        const u32x4 *src = (const u32x4 *)(a.images + (size_t)q * a.img_bytes);
        for (unsigned i = t; i < a.img_bytes / 16; i += SPARSE_RESCORE_CAND) ((u32x4 *)smem)[i] = src[i];
    }
    const int row = c < a.n_cand ? a.cand[(size_t)q * a.n_cand + c] : -1;
    bool rok = row >= 0 && row < a.n_rows;
    if (rok && a.live) rok = (a.live[row >> 5] >> (row & 31)) & 1u;
    __syncthreads();
    const size_t pf_off = (size_t)a.words * 4, qw_off = pf_off + (((size_t)a.words * 2 + 3) & ~(size_t)3);
    float acc = 0.f;
    if (rok) {
        const int n = min(a.counts[row], a.width);
        const id_t *ip = (const id_t *)a.sids + slot(row, 0, a.width);
        const w_t *wp = (const w_t *)a.sweights + slot(row, 0, a.width);
        for (int j = 0; j < n; ++j) {
            const int id = (int)ip[(size_t)j * SPARSE_BLOCK_ROWS];
            const float w = (float)wp[(size_t)j * SPARSE_BLOCK_ROWS];
            const int wi = id >> 5;
            const uint32_t bit = 1u << (id & 31);
            const uint32_t word = ((const uint32_t *)smem)[wi];
            if (word & bit) {
                const int r = (int)((const uint16_t *)(smem + pf_off))[wi] + __popc(word & (bit - 1u));
                acc = __builtin_fmaf(w, ((const float *)(smem + qw_off))[r], acc);
            }
        }
    }
    if (c < a.n_cand) {
        a.ws_s[(size_t)q * a.n_cand + c] = rok ? acc : -INFINITY;
        a.ws_i[(size_t)q * a.n_cand + c] = rok ? row : SENT_ID;
    }
}

// Compaction: one thread per slot of dst's blocks (sparse_index_kernels.h SparseGatherArgs)
template <int DTYPE>
__global__ __launch_bounds__(256) void sparse_index_gather_kernel(SparseGatherArgs a) {
    using id_t = typename Stored<DTYPE>::id_t;
    using w_t = typename Stored<DTYPE>::w_t;
    const size_t total = block_slots(a.n, a.width);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        int row, j;
        slot_decode(e, a.width, row, j);
        id_t id = (id_t)0;
        w_t w = (w_t)0.f;
        if (row < a.n) {
            const int old = a.old_ids[row], n = a.counts[old];
            if (j < n) {
                const size_t o = slot(old, j, a.width);
                id = ((const id_t *)a.sids)[o];
                w = ((const w_t *)a.sweights)[o];
            }
            if (j == 0) a.dcounts[row] = n;
        }
        ((id_t *)a.dids)[e] = id;
        ((w_t *)a.dweights)[e] = w;
    }
}

DeviceFlags g_scan_lds;

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers (sparse_index_kernels.h)
// ------------------------------------------------------------------------------------------------
void sparse_index_kernels_init() {
    scan_lds_opt_in(g_scan_lds, {SPARSE_SCAN_FAMILY(sparse_index_scan_kernel), SPARSE_SCAN_FAMILY(sparse_hybrid_scan_kernel)});
}

void launch_sparse_add(int dtype, const SparseAddArgs &a, hipStream_t s) {
    if (dtype == 1) BERT_LAUNCH(sparse_index_add_kernel<1>, dim3((unsigned)a.n), dim3(256), 0, s, a);
    else BERT_LAUNCH(sparse_index_add_kernel<0>, dim3((unsigned)a.n), dim3(256), 0, s, a);
}

void launch_sparse_query(const SparseQueryArgs &a, hipStream_t s) {
    BERT_LAUNCH(sparse_query_kernel, dim3((unsigned)a.nq), dim3(256), (size_t)a.img_bytes, s, a);
}

void launch_sparse_scan(int dtype, const SparseScanArgs &a, size_t lds, hipStream_t s) {
    SPARSE_SCAN_LAUNCH(sparse_index_scan_kernel, dtype, a, lds, s);
}

void launch_sparse_hybrid_scan(int dtype, const SparseScanArgs &a, size_t lds, hipStream_t s) {
    SPARSE_SCAN_LAUNCH(sparse_hybrid_scan_kernel, dtype, a, lds, s);
}

// (an image is at most 50 KiB — SPARSE_MAX_VOCAB —: inside the 64 KiB a launch gets unasked)
void launch_sparse_rescore(int dtype, const SparseRescoreArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)a.nq * (unsigned)a.n_chunks;
    if (dtype == 1) BERT_LAUNCH(sparse_index_rescore_kernel<1>, dim3(grid), dim3(SPARSE_RESCORE_CAND), (size_t)a.img_bytes, s, a);
    else BERT_LAUNCH(sparse_index_rescore_kernel<0>, dim3(grid), dim3(SPARSE_RESCORE_CAND), (size_t)a.img_bytes, s, a);
}

void launch_sparse_gather(int dtype, const SparseGatherArgs &a, hipStream_t s) {
    const int blocks = (int)std::min<size_t>((block_slots(a.n, a.width) + 255) / 256, 8192);
    if (dtype == 1) BERT_LAUNCH(sparse_index_gather_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
    else BERT_LAUNCH(sparse_index_gather_kernel<0>, dim3(blocks), dim3(256), 0, s, a);
}

void launch_sparse_export(int dtype, const SparseExportArgs &a, hipStream_t s) {
    const int blocks = (int)std::min<size_t>(((size_t)a.n * a.width + 255) / 256, 8192);
    if (dtype == 1) BERT_LAUNCH(sparse_index_export_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
    else BERT_LAUNCH(sparse_index_export_kernel<0>, dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace bert_hip
