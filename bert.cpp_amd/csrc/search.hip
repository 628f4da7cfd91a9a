// search.hip — the device code of the exact top-k inner-product search over an HBM-resident embedding index: the kernels and
// their launchers (search_kernels.h).  The Index class that plans and orders them is index.cpp (search.h).
//
// A search of nq queries over N rows of dim elements is a GEMM (M = queries, N = rows, K = dim) whose epilogue selects:
//   index_topk_kernel<T>  one workgroup per (query tile of 32, slice of rows).  Each wave scores a 32 x 32 block
//                         (queries x rows) per step on the matrix cores — f16 rows: v_mfma_f32_32x32x16_f16, f32 rows:
//                         v_mfma_f32_32x32x2_f32, i8 rows: v_mfma_i32_32x32x32_i8 and the two scales, b1 rows: the same MFMA over
//                         bits expanded to +1 / -1 bytes in registers and the query's scale — and a lane ends the
//                         step with one row's scores for 16 queries.  Every score
//                         is compared with its query's threshold (the k-th best of this workgroup so far, kept in registers);
//                         only the ones that beat it are pushed.  The selection — the lists and queues in LDS, the look after
//                         a step, the sort, the write of one sorted top-k list per query to the workspace — is the protocol
//                         topk_select.h states once for every selecting kernel (written out in this one: see the kernel).
//   topk_merge_kernel     one workgroup per query: the same selection (one list) over the slices' lists, then the
//                         final ids and scores.
//                         The masked instantiations (MASKED: an index with removed rows, or a search with an
//                         allow-list) read one word of each bitmap per wave and step — the wave's block is
//                         the 32 rows of that word —, score and push only the rows whose bit of live & allow is set, and
//                         skip the loads and MFMAs of a block whose combined word is zero.
//   index_rescore_kernel<T>  one wave per (query, 32 of its candidates): the rows the ids name against that one query through the
//                         same ScoreBlock (the same MFMA chain per (query, row), so the same bits as a search), scores and ids
//                         [nq][n_cand] into the workspace — id INT_MAX, score -inf for an entry that names no live row —, from
//                         which topk_merge_kernel selects.
//   index_scores_kernel<T> the dense pass of a hybrid search (hybrid.cpp): index_topk_kernel's workgroups, tiles and ScoreBlock chain
//                         without the selection — every (query, row) score of the chunk goes to a row-contiguous matrix in HBM,
//                         which the sparse index's hybrid scan reads.  Masked: only the rows whose bit is set.
//   mask_and_kernel       the word-wise AND of up to three bitmaps (the two indexes' live words, an allow-list).
//   index_probe_kernel<T>  the probed search of a partitioned index: one workgroup per (query, item), an item being one of the
//                         query's probed lists (its members' ids come from the partition's order table) or a chunk of the
//                         unassigned tail.  Each wave scores 32 members per step as the rescore kernel does, and the workgroup
//                         selects with topk_select.h's queue, one list: k entries per item reach the workspace, from
//                         which topk_merge_kernel selects.  The masked instantiation (a probed search with an allow-list)
//                         scores and pushes only the members whose bit of live & allow is set; a wave whose 32 members hold
//                         none issues no row loads and no MFMA.
//   index_export_kernel<T>  stored rows, named by id, back as f32 (ScoreBlock<T>::element): bert_hip_index_get_rows, and the
//                         queries of the partition's assignment.
//   kmeans_update_kernel<T>  one workgroup per list: the sum of its members' exported rows in an order fixed by the member
//                         positions (each wave every fourth member, then a fixed tree over the waves), divided by its norm.
//   index_gather_kernel   compaction: stored rows (and i8 scales) of the listed old ids into a fresh allocation.
//   live_set_range_kernel sets the live bits of newly added rows.
//   index_convert_kernel  f32 rows (added rows, queries) -> the stored form: f32 or f16 (RNE), zero-padded to dpad.
//   index_quantize_kernel f32 rows (added rows, queries) -> the i8 form: one wave per row, codes zero-padded to dpad and one
//                         f32 scale per row.
//   index_pack_b1_kernel  f32 rows (added rows) -> the b1 form: one wave per row, 64 sign bits per step from a ballot.
//
// The i8 form (dtype 2): a row or query x is stored as scale = amax / 127 (amax = max |x_i|; NaN if any x_i is NaN or +-inf)
// and codes c_i = clamp(rint(x_i / scale), -127, 127) (all 0 if the scale is 0 or NaN); its score is
// ((float)dot * qscale) * rscale with dot = sum_i qc_i rc_i an exact int32 (|dot| <= 2048 * 127^2 < 2^31).  A row that held a
// NaN or an inf scores NaN and is never returned; so does every row for such a query.
//
// The b1 form (dtype 3): element i of a row is bit i & 31 of u32 word i >> 5, set iff x_i > 0 (so -0, NaN and -inf give 0, +inf
// gives 1: a row's non-finite elements are not detected); dpad is a multiple of 128 (rows are whole 16-byte pieces), the padding
// bits zero, no scale.  Queries are quantized as for i8.  score = (float)dot * qscale with dot = sum_i qc_i (bit_i ? +1 : -1) an
// exact int32; the padding's -1 meets a zero code.
//
// Order of a result: larger score first, equal scores (==, so +0 equals -0) by smaller id; NaN scores never pass a compare
// and are never returned; missing entries are id -1, score -inf (inside the kernels: id INT_MAX, which ranks below every row).
// Determinism: a (query, row) score is one MFMA accumulation chain in a fixed k order that depends on nothing but dpad (i8: an
// exact integer sum, then two multiplies), and the key order is total over distinct rows, so the set and order of a result do
// not depend on the slicing, the chunking of the queries, the neighbours in a batch, or k (top-10 is the first 10 of top-100);
// nor on whether a search or a rescore computed it: both end a chain with the same ScoreBlock<T>::finish.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "device.h"
#include "score_chain.h"
#include "search_kernels.h"
#include "topk_select.h"

namespace bert_hip {

namespace {

constexpr int MERGE_U = 16;             // candidates per thread and round of the merge


// One 32 x 32 block of scores: acc[r] = query (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile against row (lane & 31).
// qp / rp: this lane's query / row (rows of dpad elements); qok / rok false: that operand is zero.  The k order of the
// accumulation is fixed by dpad alone.
// ScoreBlock<T> is also everything else a kernel knows of the stored form T: query_t / acc_t, the element of a query as run
// reads it and run's accumulator; QSCALE / RSCALE, whether a score takes the query's / the row's scale; row_ptr, stored row
// `row` of rows of dpad elements; finish, one accumulator element -> the score, the one place that arithmetic is written;
// element, element e of a stored row as f32 (rs: its scale where RSCALE) — what bert_hip_index_get_rows returns.
template <class T> struct ScoreBlock;

// f16, f32: queries are stored as rows are, and the MFMA's f32 sum is the score
template <class T> struct FloatForm {
    using query_t = T;
    using acc_t = f32x16;
    static constexpr bool QSCALE = false, RSCALE = false;
    static __device__ __forceinline__ const T *row_ptr(const void *rows, size_t row, int dpad) { return (const T *)rows + row * dpad; }
    static __device__ __forceinline__ float finish(float acc, float, float) { return acc; }
    static __device__ __forceinline__ float element(const T *rp, float, int e) { return (float)rp[e]; }
};

template <> struct ScoreBlock<half_t> : FloatForm<half_t> {
    // v_mfma_f32_32x32x16_f16: lane l holds A[l & 31][16 s + 8 (l >> 5) + j] and B[..][l & 31] in element j of step s
    static __device__ __forceinline__ void run(const half_t *qp, const half_t *rp, bool qok, bool rok, int dpad, int h, f32x16 &acc) {
        // (the chain itself: score_chain.h, shared with maxsim.hip)
        const f16x8 z = {};
        score_chain_f16([&](int k, bool in) __attribute__((always_inline)) { return qok && in ? *(const f16x8 *)(qp + k + 8 * h) : z; },
                        [&](int k, bool in) __attribute__((always_inline)) { return rok && in ? *(const f16x8 *)(rp + k + 8 * h) : z; }, dpad, acc);
    }
};

template <> struct ScoreBlock<float> : FloatForm<float> {
    // v_mfma_f32_32x32x2_f32 (an exact f32 fma chain): lane l loads the float4 at k = 8 g + 4 (l >> 5) and feeds element e
    // to step (g, e), which covers k = 8 g + e and 8 g + 4 + e
    static __device__ __forceinline__ void run(const float *qp, const float *rp, bool qok, bool rok, int dpad, int h, f32x16 &acc) {
        constexpr int U = 8;
        const f32x4 z = {};
        for (int k0 = 0; k0 < dpad; k0 += 8 * U) {
            f32x4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + 8 * u < dpad;
                const int kk = k0 + 8 * u + 4 * h;
                a[u] = qok && in ? *(const f32x4 *)(qp + kk) : z;
                b[u] = rok && in ? *(const f32x4 *)(rp + kk) : z;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 8 * u < dpad) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], b[u][0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], b[u][1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][2], b[u][2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][3], b[u][3], acc, 0, 0, 0);
                }
        }
    }
};

template <> struct ScoreBlock<int8_t> {
    using query_t = int8_t;
    using acc_t = i32x16;
    static constexpr bool QSCALE = true, RSCALE = true;
    static __device__ __forceinline__ const int8_t *row_ptr(const void *rows, size_t row, int dpad) { return (const int8_t *)rows + row * dpad; }
    // (two multiplies in this order and no add: nothing the compiler could contract)
    static __device__ __forceinline__ float finish(int dot, float qs, float rs) { return ((float)dot * qs) * rs; }
    static __device__ __forceinline__ float element(const int8_t *rp, float rs, int e) { return (float)rp[e] * rs; }
    // v_mfma_i32_32x32x32_i8: lane l feeds the 16 bytes at k = 32 s + 16 (l >> 5) of its query and of its row to step s — the
    // same k map on both sides, and an integer sum is exact in any order
    static __device__ __forceinline__ void run(const int8_t *qp, const int8_t *rp, bool qok, bool rok, int dpad, int h, i32x16 &acc) {
        constexpr int U = 8;
        const i32x4 z = {};
        for (int k0 = 0; k0 < dpad; k0 += 32 * U) {
            i32x4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + 32 * u < dpad;
                const int kk = k0 + 32 * u + 16 * h;
                a[u] = qok && in ? *(const i32x4 *)(qp + kk) : z;
                b[u] = rok && in ? *(const i32x4 *)(rp + kk) : z;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 32 * u < dpad) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u], b[u], acc, 0, 0, 0);
        }
    }
};

// a stored byte of a b1 row: the sign bits of eight elements
struct b1_t { uint8_t bits; };

template <> struct ScoreBlock<b1_t> {
    using query_t = int8_t;
    using acc_t = i32x16;
    static constexpr bool QSCALE = true, RSCALE = false;
    // (dpad / 8 bytes per row)
    static __device__ __forceinline__ const b1_t *row_ptr(const void *rows, size_t row, int dpad) { return (const b1_t *)rows + row * (dpad >> 3); }
    static __device__ __forceinline__ float finish(int dot, float qs, float) { return (float)dot * qs; }
    static __device__ __forceinline__ float element(const b1_t *rp, float, int e) { return (rp[e >> 3].bits >> (e & 7)) & 1 ? 1.f : -1.f; }
    // bit 4 j + b of bits16 in byte b of element j: 0x01 for a set bit, 0xff (-1) for a clear one.  The multiply puts bit b of
    // a nibble at bit 8 b (four copies 7 bits apart, which do not overlap); the byte permute looks 0 / 1 up in {0xff, 0x01}
    static __device__ __forceinline__ i32x4 expand(uint32_t bits16) {
        i32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t t = (((bits16 >> (4 * j)) & 0xfu) * 0x00204081u) & 0x01010101u;
            v[j] = (int)__builtin_amdgcn_perm(0x000001ffu, 0x000001ffu, t);
        }
        return v;
    }
    // v_mfma_i32_32x32x32_i8, the row operand dequantised in the tile load: lane l feeds step s the query's 16 codes at
    // k = 32 s + 16 (l >> 5) and the row's bits at the same k — half (l >> 5) of its word s — as sixteen +-1 bytes.  A 16-byte
    // load of the row serves four steps.  (rok false: the row's scores mean nothing — no caller reads them; the bits are
    // not loaded.)
    static __device__ __forceinline__ void run(const int8_t *qp, const b1_t *rp, bool qok, bool rok, int dpad, int h, i32x16 &acc) {
        constexpr int U = 2;
        const i32x4 z = {};
        const u32x4 zw = {};
        for (int k0 = 0; k0 < dpad; k0 += 128 * U) {
            i32x4 a[U][4];
            u32x4 w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + 128 * u < dpad;
                w[u] = rok && in ? *(const u32x4 *)(rp + ((k0 + 128 * u) >> 3)) : zw;
#pragma unroll
                for (int t = 0; t < 4; ++t) a[u][t] = qok && in ? *(const i32x4 *)(qp + k0 + 128 * u + 32 * t + 16 * h) : z;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 128 * u < dpad) {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u][t], expand((w[u][t] >> (16 * h)) & 0xffffu), acc, 0, 0, 0);
                }
        }
    }
};

// LDS: float scores [nqv][L], int ids [nqv][L], int count [nqv] — per query the current top-k in [0, k), the queue behind
// The selection is written out here, not taken from topk_select.h's helpers: with them this kernel measured slower.
// The protocol and its barrier contract are the ones stated there.
template <class T, bool MASKED>
__global__ __launch_bounds__(NT) void index_topk_kernel(TopkArgs a) {
    using F = ScoreBlock<T>;
    using QE = typename F::query_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int item = xcd_item();                 // (kernels.h: the query tiles of one slice of rows go to one XCD)
    if (item >= a.n_items) return;
    const int slice = item / a.n_qtiles, qt = item - slice * a.n_qtiles;
    const int q0 = qt * QT, nqv = min(QT, a.nq - q0);
    const int r0 = slice * a.slice_rows, r1 = min(a.n_rows, r0 + a.slice_rows);
    const int L = a.L, k = a.k;
    float *ls = (float *)smem;
    int *li = (int *)(ls + nqv * L);
    int *cnt = li + nqv * L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;

    for (int i = tid; i < nqv * L; i += NT) { ls[i] = -INFINITY; li[i] = SENT_ID; }
    if (tid < nqv) cnt[tid] = 0;
    float ts[16];
    int ti[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { ts[r] = -INFINITY; ti[r] = SENT_ID; }
    // the scales of this lane's 16 queries (a form without them: zeros nobody reads)
    float qs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
        qs[r] = F::QSCALE && q < nqv ? a.qscale[q0 + q] : 0.f;
    }
    __syncthreads();

    const bool qok = col < nqv;
    const QE *qp = (const QE *)a.queries + (size_t)(q0 + (qok ? col : 0)) * a.dpad;
    // a step pushes at most STEP_ROWS entries per query: sort before a queue could hold fewer free slots
    const int room = L - k - STEP_ROWS;
    for (int base = r0; base < r1; base += STEP_ROWS) {
        const int row = base + wave * 32 + col;
        bool rok = row < r1;
        // masked: r0 and the step are multiples of 128, so the wave's 32 rows are the bits of one word, the same for all
        // its lanes; a block that starts at or beyond r1 has no word
        [[maybe_unused]] uint32_t word = 0;
        if constexpr (MASKED) {
            const int blk = __builtin_amdgcn_readfirstlane(base + wave * 32);
            if (blk < r1) {
                word = ~0u;
                if (a.live) word &= a.live[blk >> 5];
                if (a.allow) word &= a.allow[blk >> 5];
            }
            word = __builtin_amdgcn_readfirstlane(word);
            rok = rok && ((word >> col) & 1u);           // (a row that does not qualify is a zero operand and never pushed)
        }
        f32x16 acc = {};
        // (masked: a block without a qualifying row costs no loads and no MFMAs — wave-uniform, and the barriers are below)
        if (!MASKED || word != 0) {
            const T *rp = F::row_ptr(a.rows, (size_t)(rok ? row : r0), a.dpad);
            const float rs = F::RSCALE ? a.rscale[rok ? row : r0] : 0.f;
            typename F::acc_t dot = {};
            F::run(qp, rp, qok, rok, a.dpad, h, dot);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = F::finish(dot[r], qs[r], rs);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
            const float s = acc[r];
            if (rok && q < nqv && better(s, row, ts[r], ti[r])) {
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
            for (int r = 0; r < 16; ++r) {
                const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
                if (q < nqv) { ts[r] = ls[q * L + k - 1]; ti[r] = li[q * L + k - 1]; }
            }
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

// LDS: float scores [L], int ids [L], int count
__global__ __launch_bounds__(NT) void topk_merge_kernel(MergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int L = a.L, k = a.k, tid = threadIdx.x;
    float *ls = (float *)smem;
    int *li = (int *)(ls + L);
    const SelectLists sel{ls, li, li + L, L, k, L - k - NT};       // a look follows at most NT pushes
    const float *cs = a.ws_s + (size_t)blockIdx.x * a.n_cand;
    const int *ci = a.ws_i + (size_t)blockIdx.x * a.n_cand;
    select_init(sel, 1, tid);
    float ts = -INFINITY;
    int ti = SENT_ID;
    __syncthreads();
    for (int base = 0; base < a.n_cand; base += NT * MERGE_U) {
        float s[MERGE_U];
        int id[MERGE_U];
#pragma unroll
        for (int u = 0; u < MERGE_U; ++u) {
            const int c = base + u * NT + tid;
            s[u] = c < a.n_cand ? cs[c] : -INFINITY;
            id[u] = c < a.n_cand ? ci[c] : SENT_ID;
        }
#pragma unroll
        for (int u = 0; u < MERGE_U; ++u) {
            if (better(s[u], id[u], ts, ti)) select_push(sel, 0, s[u], id[u]);
            // (a look per u, not per round: a round's MERGE_U * NT candidates would not fit behind the top-k)
            if (select_step_end(sel, 1, tid)) {
                select_threshold(sel, 0, ts, ti);
                select_resume(sel, 1, tid);
            }
        }
    }
    select_finish(sel, 1, tid);
    for (int j = tid; j < k; j += NT) {
        const int id = li[j];
        a.ids[(size_t)blockIdx.x * k + j] = id == SENT_ID ? -1 : id;
        a.scores[(size_t)blockIdx.x * k + j] = ls[j];
    }
}

// One wave per (query, block of 32 of its candidates): the block's rows are the MFMA's 32 rows, the query is query 0 of the
// tile (the other 31 are zero operands), so lane l < 32 ends with acc[0] = its row's score — the accumulation chain of a search.
template <class T>
__global__ __launch_bounds__(NT) void index_rescore_kernel(RescoreArgs a) {
    using F = ScoreBlock<T>;
    using QE = typename F::query_t;
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const int w = (int)blockIdx.x * NWAVE + (int)(threadIdx.x >> 6);
    if (w >= a.nq * a.n_blocks) return;                        // (the whole wave)
    const int q = w / a.n_blocks, c = (w - q * a.n_blocks) * 32 + col;
    const int id = c < a.n_cand ? a.cand[(size_t)q * a.n_cand + c] : -1;
    bool rok = id >= 0 && id < a.n_rows;
    if (rok && a.live) rok = (a.live[id >> 5] >> (id & 31)) & 1u;
    float s = -INFINITY;
    if (__any(rok)) {                                          // (wave-uniform)
        const bool qok = col == 0;
        const QE *qp = (const QE *)a.queries + (size_t)q * a.dpad;
        const T *rp = F::row_ptr(a.rows, (size_t)(rok ? id : 0), a.dpad);
        const float rs = F::RSCALE && rok ? a.rscale[id] : 0.f;
        typename F::acc_t dot = {};
        F::run(qp, rp, qok, rok, a.dpad, h, dot);
        s = F::finish(dot[0], F::QSCALE ? a.qscale[q] : 0.f, rs);
    }
    if (h == 0 && c < a.n_cand) {
        a.ws_s[(size_t)q * a.n_cand + c] = rok ? s : -INFINITY;
        a.ws_i[(size_t)q * a.n_cand + c] = rok ? id : SENT_ID;
    }
}

// index_topk_kernel without the selection: one workgroup of four waves per (tile of QT queries, slice of rows), the same item map;
// each wave scores 32 rows a step through ScoreBlock<T>::run and finish — the search's bits — and stores acc[r] to
// out[(q0 + q) * ld + row] for the queries q < nqv: per accumulator element the 32 lanes of a half-wave write 32 consecutive floats.
// No LDS, no barrier: a wave whose block lies beyond the slice, or (MASKED) holds no row whose bit of mask is set, does nothing;
// a row whose bit is clear is a zero operand and is not written.  No word at or beyond ceil(n_rows / 32) is read.
template <class T, bool MASKED>
__global__ __launch_bounds__(NT) void index_scores_kernel(ScoresArgs a) {
    using F = ScoreBlock<T>;
    using QE = typename F::query_t;
    const int item = xcd_item();
    if (item >= a.n_items) return;
    const int slice = item / a.n_qtiles, qt = item - slice * a.n_qtiles;
    const int q0 = qt * QT, nqv = min(QT, a.nq - q0);
    const int r0 = slice * a.slice_rows, r1 = min(a.n_rows, r0 + a.slice_rows);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    float qs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
        qs[r] = F::QSCALE && q < nqv ? a.qscale[q0 + q] : 0.f;
    }
    const bool qok = col < nqv;
    const QE *qp = (const QE *)a.queries + (size_t)(q0 + (qok ? col : 0)) * a.dpad;
    for (int base = r0; base < r1; base += STEP_ROWS) {
        const int blk = __builtin_amdgcn_readfirstlane(base + wave * 32);
        if (blk >= r1) continue;                               // (the whole wave)
        const int row = blk + col;
        bool rok = row < r1;
        if constexpr (MASKED) {
            // r0 and the step are multiples of 128: the wave's 32 rows are the bits of one word
            const uint32_t word = __builtin_amdgcn_readfirstlane(a.mask[blk >> 5]);
            if (word == 0) continue;
            rok = rok && ((word >> col) & 1u);
        }
        const T *rp = F::row_ptr(a.rows, (size_t)(rok ? row : r0), a.dpad);
        const float rs = F::RSCALE ? a.rscale[rok ? row : r0] : 0.f;
        typename F::acc_t dot = {};
        F::run(qp, rp, qok, rok, a.dpad, h, dot);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
            if (rok && q < nqv) a.out[(size_t)(q0 + q) * a.ld + row] = F::finish(dot[r], qs[r], rs);
        }
    }
}

// One thread per word
__global__ __launch_bounds__(256) void mask_and_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                       const uint32_t *__restrict__ c, uint32_t *__restrict__ out, int n_words) {
    const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= n_words) return;
    uint32_t m = ~0u;
    if (a) m &= a[w];
    if (b) m &= b[w];
    if (c) m &= c[w];
    out[w] = m;
}

// One workgroup per (query, item); the item's members m0 .. m1 - 1 are rows order[m] (a probed list) or m itself (a tail chunk).
// Scoring is index_rescore_kernel's — the query is query 0 of the tile, lane l < 32 ends with its member's score —, selection
// topk_select.h's with one list.  The k entries written for an item that has fewer candidates are (-inf, SENT_ID).
// MASKED (a search with an allow-list): a member is a candidate iff its bit of live & allow is set.  The members of a list are
// scattered ids, so each lane reads its own member's words; the members of a tail chunk are consecutive ids, so the wave's 32
// bits come from at most two words read once per wave and step (the tail starts at n_part, any row: the block straddles two
// words unless it happens to start at a multiple of 32).  A word that holds no row below n_rows is never read.
template <class T, bool MASKED>
__global__ __launch_bounds__(NT) void index_probe_kernel(ProbeArgs a) {
    using F = ScoreBlock<T>;
    using QE = typename F::query_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int q = (int)blockIdx.x / a.n_items, item = (int)blockIdx.x - q * a.n_items;
    const int L = a.L, k = a.k, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    float *ls = (float *)smem;
    int *li = (int *)(ls + L);
    const SelectLists sel{ls, li, li + L, L, k, L - k - STEP_ROWS};        // a step pushes at most STEP_ROWS entries
    // (everything up to the loop is uniform over the workgroup)
    const bool listed = item < a.nprobe;
    int m0 = 0, m1 = 0;
    if (listed) {
        const int l = a.probe[(size_t)q * a.nprobe + item];
        if (l >= 0 && l < a.n_lists) { m0 = a.offsets[l]; m1 = a.offsets[l + 1]; }
    } else {
        // (64-bit: n_part + c * PROBE_CHUNK may pass 2^31 in the last chunk's end)
        const long long t0 = (long long)a.n_part + (long long)(item - a.nprobe) * PROBE_CHUNK;
        m0 = (int)min(t0, (long long)a.n_rows);
        m1 = (int)min(t0 + PROBE_CHUNK, (long long)a.n_rows);
    }
    const size_t out = ((size_t)q * a.n_items + item) * k;
    if (m0 >= m1) {
        select_store_empty(a.ws_s, a.ws_i, out, k, tid);
        return;
    }
    const QE *qp = (const QE *)a.queries + (size_t)q * a.dpad;
    const float qs = F::QSCALE ? a.qscale[q] : 0.f;
    select_init(sel, 1, tid);
    float ts = -INFINITY;
    int ti = SENT_ID;
    __syncthreads();

    // (the trip count is the workgroup's: the barriers below are met by every wave)
    for (int base = m0; base < m1; base += STEP_ROWS) {
        const int m = base + wave * 32 + col;
        const int id = m < m1 ? (listed ? a.order[m] : m) : -1;
        bool rok = id >= 0 && id < a.n_rows;
        if constexpr (!MASKED) {
            if (rok && a.live) rok = (a.live[id >> 5] >> (id & 31)) & 1u;
        } else if (listed) {
            if (rok) {
                uint32_t w = a.allow[id >> 5];
                if (a.live) w &= a.live[id >> 5];
                rok = (w >> (id & 31)) & 1u;
            }
        } else {
            // the wave's block is rows b0 .. b0 + 31: bit c of `bits` is row b0 + c's, from word b0 >> 5 and, where the block
            // straddles and the next word still holds a row below m1 (<= n_rows), from that one
            const int b0 = __builtin_amdgcn_readfirstlane(base + wave * 32);
            uint32_t bits = 0;
            if (b0 < m1) {
                const int w0 = b0 >> 5, sh = b0 & 31;
                uint32_t lo = a.allow[w0];
                if (a.live) lo &= a.live[w0];
                bits = lo >> sh;
                if (sh != 0 && w0 < ((m1 - 1) >> 5)) {
                    uint32_t hi = a.allow[w0 + 1];
                    if (a.live) hi &= a.live[w0 + 1];
                    bits |= hi << (32 - sh);
                }
            }
            bits = __builtin_amdgcn_readfirstlane(bits);
            rok = rok && ((bits >> col) & 1u);
        }
        if (__any(rok)) {                                          // (wave-uniform)
            const T *rp = F::row_ptr(a.rows, (size_t)(rok ? id : 0), a.dpad);
            const float rs = F::RSCALE && rok ? a.rscale[id] : 0.f;
            typename F::acc_t dot = {};
            F::run(qp, rp, col == 0, rok, a.dpad, h, dot);
            const float s = F::finish(dot[0], qs, rs);
            if (h == 0 && rok && better(s, id, ts, ti)) select_push(sel, 0, s, id);
        }
        if (select_step_end(sel, 1, tid)) {
            select_threshold(sel, 0, ts, ti);
            select_resume(sel, 1, tid);
        }
    }
    select_finish(sel, 1, tid);
    for (int j = tid; j < k; j += NT) { a.ws_s[out + j] = ls[j]; a.ws_i[out + j] = li[j]; }
}

template <class T>
__global__ __launch_bounds__(256) void index_export_kernel(ExportArgs a) {
    using F = ScoreBlock<T>;
    const size_t total = (size_t)a.n * a.dim;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / a.dim;
        const int c = (int)(i - r * a.dim);
        const size_t row = a.ids ? (size_t)a.ids[r] : (size_t)a.first + r;
        a.out[i] = F::element(F::row_ptr(a.rows, row, a.dpad), F::RSCALE ? a.rscale[row] : 0.f, c);
    }
}

// One workgroup per list.  Lane l of a wave owns elements l, l + 64, ... of the sum; wave w adds members w, w + NWAVE, ... of the
// list in that order, the four partial sums meet as (0 + 1) + (2 + 3), and the squares as each thread's elements in ascending
// order, then a halving tree over the threads: the bits depend on the member positions alone.  No atomics.
template <class T>
__global__ __launch_bounds__(NT) void kmeans_update_kernel(KmeansArgs a) {
    using F = ScoreBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int EPL = 2048 / 64;               // elements per lane at the largest dim of an index
    float *part = (float *)smem;                 // [NWAVE][dim], then [dim] the sum
    float *sq = part + NWAVE * a.dim;            // [NT]
    const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, dim = a.dim;
    const int m0 = a.offsets[l], m1 = a.offsets[l + 1];
    if (m0 >= m1) return;                        // (the whole workgroup)
    float acc[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc[j] = 0.f;
    for (int m = m0 + wave; m < m1; m += NWAVE) {
        const int row = a.order[m];
        const T *rp = F::row_ptr(a.rows, (size_t)row, a.dpad);
        const float rs = F::RSCALE ? a.rscale[row] : 0.f;
#pragma unroll
        for (int j = 0; j < EPL; ++j)
            if (64 * j + lane < dim) acc[j] += F::element(rp, rs, 64 * j + lane);
    }
#pragma unroll
    for (int j = 0; j < EPL; ++j)
        if (64 * j + lane < dim) part[wave * dim + 64 * j + lane] = acc[j];
    __syncthreads();
    float ss = 0.f;
    for (int e = tid; e < dim; e += NT) {
        const float v = (part[e] + part[dim + e]) + (part[2 * dim + e] + part[3 * dim + e]);
        part[e] = v;
        ss += v * v;
    }
    sq[tid] = ss;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) sq[tid] += sq[tid + o];
        __syncthreads();
    }
    const float norm = sqrtf(sq[0]);
    if (!(norm > 0.f) || !__builtin_isfinite(norm)) return;
    for (int e = tid; e < dim; e += NT) a.centroids[(size_t)l * dim + e] = part[e] / norm;
}

template <class T>
__global__ __launch_bounds__(256) void index_convert_kernel(const float *__restrict__ src, T *__restrict__ dst, int n, int dim, int dpad) {
    const size_t total = (size_t)n * dpad;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / dpad;
        const int c = (int)(i - r * dpad);
        dst[i] = c < dim ? (T)src[r * dim + c] : (T)0;        // (float -> _Float16: round to nearest even)
    }
}

// f32 rows [n][dim] -> i8 codes [n][dpad] and scales [n] (the i8 form above).  One wave per row, by device.h's quantize_row_i8.
__global__ __launch_bounds__(256) void index_quantize_kernel(const float *__restrict__ src, int8_t *__restrict__ codes,
                                                             float *__restrict__ scales, int n, int dim, int dpad) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)n) return;                                // (the whole wave)
    quantize_row_i8(src + r * dim, dim, dpad, codes + r * dpad, scales + r, lane);
}

// f32 rows [n][dim] -> b1 rows [n][dpad / 32] words (the b1 form above).  One wave per row: a ballot of x > 0 is the 64 bits of
// elements c0 .. c0 + 63, whose two words lanes 0 and 1 store.  dpad is a multiple of 128; elements at and beyond dim are 0.
__global__ __launch_bounds__(256) void index_pack_b1_kernel(const float *__restrict__ src, uint32_t *__restrict__ dst, int n, int dim, int dpad) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)n) return;                                // (the whole wave)
    const float *x = src + r * dim;
    uint32_t *out = dst + r * (size_t)(dpad >> 5);
    for (int c0 = 0; c0 < dpad; c0 += 64) {
        const float v = c0 + lane < dim ? x[c0 + lane] : 0.f;
        const unsigned long long m = __ballot(v > 0.f);        // (an IEEE compare: false for -0, NaN, -inf)
        if (lane < 2) out[(c0 >> 5) + lane] = (uint32_t)(m >> (32 * lane));
    }
}

// Compaction: row i of dst (row_bytes, a multiple of 16) = row old_ids[i] of src, and the i8 scale with it (sscale null for
// the other forms).  One thread per 16-byte piece.
__global__ __launch_bounds__(256) void index_gather_kernel(const i32x4 *__restrict__ src, i32x4 *__restrict__ dst,
                                                           const float *__restrict__ sscale, float *__restrict__ dscale,
                                                           const int32_t *__restrict__ old_ids, int n, int pieces) {
    const size_t total = (size_t)n * pieces;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / pieces;
        const int c = (int)(i - r * pieces);
        const size_t o = (size_t)old_ids[r];
        dst[i] = src[o * pieces + c];
        if (sscale && c == 0) dscale[r] = sscale[o];
    }
}

// live bits of rows [first, first + n) := 1.  One thread per word of the range, read-modify-write: the index's operations
// never overlap, and no two threads share a word.
__global__ __launch_bounds__(256) void live_set_range_kernel(uint32_t *__restrict__ live, int first, int n) {
    const int w0 = first >> 5, w1 = (int)(((long long)first + n - 1) >> 5);
    const int w = w0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w > w1) return;
    uint32_t m = ~0u;
    if (w == w0) m &= ~0u << (first & 31);
    const int last = (int)(((long long)first + n - 1) & 31);
    if (w == w1 && last < 31) m &= (1u << (last + 1)) - 1u;
    live[w] |= m;
}

// f(ScoreBlock<T>{}) for the T of dtype
template <class Fn> void dispatch(int dtype, Fn &&f) {
    switch (dtype) {
    case 3: return f(ScoreBlock<b1_t>{});
    case 2: return f(ScoreBlock<int8_t>{});
    case 1: return f(ScoreBlock<half_t>{});
    default: return f(ScoreBlock<float>{});
    }
}
template <class T> T row_type(ScoreBlock<T>);

}  // namespace

// ------------------------------------------------------------------------------------------------
// launchers (search_kernels.h)
// ------------------------------------------------------------------------------------------------
void search_kernels_init() {
    // (128 KiB of LDS, beyond the 64 KiB a launch gets unasked; a launch that still cannot have it fails, and the search
    // reports the launch error)
    const int lds_max = QT * 512 * 8 + QT * 4;
    for (int dtype = 0; dtype < 4; ++dtype)
        dispatch(dtype, [&](auto form) {
            using T = decltype(row_type(form));
            (void)hipFuncSetAttribute((const void *)index_topk_kernel<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
            (void)hipFuncSetAttribute((const void *)index_topk_kernel<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        });
}

void launch_topk(int dtype, const TopkArgs &a, size_t lds, hipStream_t s) {
    const int grid = xcd_grid(a.n_items);
    dispatch(dtype, [&](auto form) {
        using T = decltype(row_type(form));
        if (a.live || a.allow) BERT_LAUNCH((index_topk_kernel<T, true>), dim3(grid), dim3(NT), lds, s, a);
        else BERT_LAUNCH((index_topk_kernel<T, false>), dim3(grid), dim3(NT), lds, s, a);
    });
}

void launch_topk_merge(const MergeArgs &a, int nq, hipStream_t s) {
    BERT_LAUNCH(topk_merge_kernel, dim3(nq), dim3(NT), (size_t)a.L * 8 + 16, s, a);
}

void launch_rescore(int dtype, const RescoreArgs &a, hipStream_t s) {
    const int grid = (a.nq * a.n_blocks + NWAVE - 1) / NWAVE;
    dispatch(dtype, [&](auto form) { BERT_LAUNCH(index_rescore_kernel<decltype(row_type(form))>, dim3(grid), dim3(NT), 0, s, a); });
}

void launch_index_scores(int dtype, const ScoresArgs &a, hipStream_t s) {
    const int grid = xcd_grid(a.n_items);
    dispatch(dtype, [&](auto form) {
        using T = decltype(row_type(form));
        if (a.mask) BERT_LAUNCH((index_scores_kernel<T, true>), dim3(grid), dim3(NT), 0, s, a);
        else BERT_LAUNCH((index_scores_kernel<T, false>), dim3(grid), dim3(NT), 0, s, a);
    });
}

void launch_mask_and(const uint32_t *a, const uint32_t *b, const uint32_t *c, uint32_t *out, int n_words, hipStream_t s) {
    BERT_LAUNCH(mask_and_kernel, dim3((n_words + 255) / 256), dim3(256), 0, s, a, b, c, out, n_words);
}

void launch_probe(int dtype, const ProbeArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)a.nq * a.n_items);
    const size_t lds = (size_t)a.L * 8 + 16;
    dispatch(dtype, [&](auto form) {
        using T = decltype(row_type(form));
        if (a.allow) BERT_LAUNCH((index_probe_kernel<T, true>), grid, dim3(NT), lds, s, a);
        else BERT_LAUNCH((index_probe_kernel<T, false>), grid, dim3(NT), lds, s, a);
    });
}

void launch_export(int dtype, const ExportArgs &a, hipStream_t s) {
    const int blocks = (int)std::min<size_t>(((size_t)a.n * a.dim + 255) / 256, 8192);
    dispatch(dtype, [&](auto form) { BERT_LAUNCH(index_export_kernel<decltype(row_type(form))>, dim3(blocks), dim3(256), 0, s, a); });
}

void launch_kmeans_update(int dtype, const KmeansArgs &a, hipStream_t s) {
    const size_t lds = ((size_t)NWAVE * a.dim + NT) * 4;
    dispatch(dtype, [&](auto form) { BERT_LAUNCH(kmeans_update_kernel<decltype(row_type(form))>, dim3(a.n_lists), dim3(NT), lds, s, a); });
}

void launch_ingest(int dtype, const float *src, void *dst, float *scales, int n, int dim, int dpad, hipStream_t s) {
    const int blocks = (int)std::min<size_t>(((size_t)n * dpad + 255) / 256, 8192);
    switch (dtype) {
    case 3: BERT_LAUNCH(index_pack_b1_kernel, dim3((n + 3) / 4), dim3(256), 0, s, src, (uint32_t *)dst, n, dim, dpad); break;
    case 2: BERT_LAUNCH(index_quantize_kernel, dim3((n + 3) / 4), dim3(256), 0, s, src, (int8_t *)dst, scales, n, dim, dpad); break;
    case 1: BERT_LAUNCH(index_convert_kernel<half_t>, dim3(blocks), dim3(256), 0, s, src, (half_t *)dst, n, dim, dpad); break;
    default: BERT_LAUNCH(index_convert_kernel<float>, dim3(blocks), dim3(256), 0, s, src, (float *)dst, n, dim, dpad); break;
    }
}

void launch_gather(const void *src, void *dst, const float *sscale, float *dscale, const int32_t *old_ids, int n, size_t row_bytes, hipStream_t s) {
    const int pieces = (int)(row_bytes / 16);
    const int blocks = (int)std::min<size_t>(((size_t)n * pieces + 255) / 256, 16384);
    BERT_LAUNCH(index_gather_kernel, dim3(blocks), dim3(256), 0, s, (const i32x4 *)src, (i32x4 *)dst, sscale, dscale, old_ids, n, pieces);
}

void launch_live_set_range(uint32_t *live, int first, int n, hipStream_t s) {
    const int words = (int)(((long long)first + n - 1) >> 5) - (first >> 5) + 1;
    BERT_LAUNCH(live_set_range_kernel, dim3((words + 255) / 256), dim3(256), 0, s, live, first, n);
}

}  // namespace bert_hip
