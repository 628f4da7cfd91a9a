// search.hip — exact top-k inner-product search over an HBM-resident embedding index (search.h).
//
// A search of nq queries over N rows of dim elements is a GEMM (M = queries, N = rows, K = dim) whose epilogue selects:
//   index_topk_kernel<T>  one workgroup per (query tile of 32, slice of rows).  Each wave scores a 32 x 32 block
//                         (queries x rows) per step on the matrix cores — f16 rows: v_mfma_f32_32x32x16_f16, f32 rows:
//                         v_mfma_f32_32x32x2_f32, i8 rows: v_mfma_i32_32x32x32_i8 and the two scales, b1 rows: the same MFMA over
//                         bits expanded to +1 / -1 bytes in registers and the query's scale — and a lane ends the
//                         step with one row's scores for 16 queries.  Every score
//                         is compared with its query's threshold (the k-th best of this workgroup so far, kept in registers);
//                         only the ones that beat it go into the query's candidate queue in LDS (an LDS atomic hands out the
//                         slot).  When a queue might not take another step's rows, the lists are bitonic-sorted in LDS by
//                         (score, id) keys, the first k kept and the thresholds raised.  At the end of its slice the
//                         workgroup writes one sorted top-k list per query to the workspace.
//   topk_merge_kernel     one workgroup per query: the same threshold / queue / sort over the slices' lists, then the
//                         final ids and scores.
//                         The masked instantiations (TopkArgsMasked / TopkArgsI8Masked / TopkArgsB1Masked: an index with removed rows, or a
//                         search with an allow-list) read one word of each bitmap per wave and step — the wave's block is
//                         the 32 rows of that word —, score and push only the rows whose bit of live & allow is set, and
//                         skip the loads and MFMAs of a block whose combined word is zero.
//   index_rescore_kernel<T>  one wave per (query, 32 of its candidates): the rows the ids name against that one query through the
//                         same ScoreBlock (the same MFMA chain per (query, row), so the same bits as a search), scores and ids
//                         [nq][n_cand] into the workspace — id INT_MAX, score -inf for an entry that names no live row —, from
//                         which topk_merge_kernel selects.
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
// nor on whether a search or a rescore computed it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "device.h"
#include "search.h"

#define HIP_OK(expr, errvar, ret)                                                                       \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            errvar = std::string(#expr) + ": " + hipGetErrorString(e__);                                \
            return ret;                                                                                 \
        }                                                                                               \
    } while (0)

namespace bert_hip {

namespace {

constexpr int QT = 32;                  // queries per workgroup tile: the M side of one 32 x 32 MFMA block
constexpr int NWAVE = 4;
constexpr int NT = 64 * NWAVE;
constexpr int STEP_ROWS = 32 * NWAVE;   // rows a workgroup scores per step (each wave one 32-row block)
constexpr int SENT_ID = INT_MAX;        // id of an empty list entry (score -inf): ranks below every row
constexpr int TARGET_BLOCKS = 2048;     // score workgroups a search aims for (8 per CU)
constexpr int MERGE_U = 16;             // candidates per thread and round of the merge


// (s, i) ranks before (ts, ti)
__device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

// Sorts nl lists of L (pow2) keys each, best first, with all NT threads of the workgroup.  Enter after a barrier; ends
// with one.
__device__ void bitonic_sort_lists(float *ls, int *li, int nl, int L, int tid) {
    const int lg_half = __builtin_ctz((unsigned)L) - 1, total = nl << lg_half;
    for (int size = 2; size <= L; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int lg_s = __builtin_ctz((unsigned)stride);
            for (int p = tid; p < total; p += NT) {
                const int list = p >> lg_half, i = p & ((1 << lg_half) - 1);
                const int lo = ((i >> lg_s) << (lg_s + 1)) + (i & (stride - 1)), hi = lo + stride;
                float *s = ls + list * L;
                int *d = li + list * L;
                const float sl = s[lo], sh = s[hi];
                const int il = d[lo], ih = d[hi];
                const bool swap = (lo & size) == 0 ? better(sh, ih, sl, il) : better(sl, il, sh, ih);
                if (swap) { s[lo] = sh; s[hi] = sl; d[lo] = ih; d[hi] = il; }
            }
            __syncthreads();
        }
}

// One 32 x 32 block of scores: acc[r] = query (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile against row (lane & 31).
// qp / rp: this lane's query / row (rows of dpad elements); qok / rok false: that operand is zero.  The k order of the
// accumulation is fixed by dpad alone.
template <class T> struct ScoreBlock;

template <> struct ScoreBlock<half_t> {
    // v_mfma_f32_32x32x16_f16: lane l holds A[l & 31][16 s + 8 (l >> 5) + j] and B[..][l & 31] in element j of step s
    static __device__ __forceinline__ void run(const half_t *qp, const half_t *rp, bool qok, bool rok, int dpad, int h, f32x16 &acc) {
        constexpr int U = 8;
        const f16x8 z = {};
        for (int k0 = 0; k0 < dpad; k0 += 16 * U) {
            f16x8 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = k0 + 16 * u < dpad;
                const int kk = k0 + 16 * u + 8 * h;
                a[u] = qok && in ? *(const f16x8 *)(qp + kk) : z;
                b[u] = rok && in ? *(const f16x8 *)(rp + kk) : z;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (k0 + 16 * u < dpad) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[u], b[u], acc, 0, 0, 0);
        }
    }
};

template <> struct ScoreBlock<float> {
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

// the element type of a query as the score block reads it, and the bytes of a stored row of dpad elements
template <class T> struct QueryElem { using type = T; };
template <> struct QueryElem<b1_t> { using type = int8_t; };
// stored row `row` of rows of dpad elements (b1: dpad / 8 bytes)
template <class T> __device__ __forceinline__ const T *row_ptr(const void *rows, size_t row, int dpad) {
    if constexpr (std::is_same_v<T, b1_t>) return (const T *)rows + row * (dpad >> 3);
    else return (const T *)rows + row * dpad;
}

struct TopkArgs {
    const void *rows, *queries;          // [n_rows][dpad], [nq][dpad] of T (b1: rows of dpad bits, queries of dpad i8 codes)
    float *ws_s;                         // [nq][n_slices][k] per-(query, slice) lists, best first
    int *ws_i;
    int n_rows, dpad, nq, n_qtiles, n_slices, slice_rows, k, L, n_items;
};
// (a type of its own: the f16 and f32 kernels keep their argument block, and with it their machine code)
struct TopkArgsI8 : TopkArgs {
    const float *qscale, *rscale;        // [nq], [n_rows]
};

// (b1: a query scale and no row scale)
struct TopkArgsB1 : TopkArgs {
    const float *qscale;                 // [nq]
};

// (types of their own again: the kernels above keep their argument blocks.)  live, allow: words [ceil(n_rows / 32)],
// bit b of word w set = row 32 w + b is live / may be returned; either may be null = all ones
struct TopkArgsMasked : TopkArgs {
    const uint32_t *live, *allow;
};
struct TopkArgsI8Masked : TopkArgsI8 {
    const uint32_t *live, *allow;
};
struct TopkArgsB1Masked : TopkArgsB1 {
    const uint32_t *live, *allow;
};
template <class Args> constexpr bool is_masked_v = std::is_same_v<Args, TopkArgsMasked> || std::is_same_v<Args, TopkArgsI8Masked> ||
                                                   std::is_same_v<Args, TopkArgsB1Masked>;

// LDS: float scores [nqv][L], int ids [nqv][L], int count [nqv] — per query the current top-k in [0, k), the queue behind
// (Args: TopkArgsI8 for T = int8_t, TopkArgsB1 for b1_t, TopkArgs otherwise; their masked forms)
template <class T, class Args>
__global__ __launch_bounds__(NT) void index_topk_kernel(Args a) {
    constexpr bool I8 = std::is_same_v<T, int8_t>, B1 = std::is_same_v<T, b1_t>, MASKED = is_masked_v<Args>;
    using QE = typename QueryElem<T>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // workgroup b runs on XCD b % 8: consecutive items — the query tiles of one slice of rows — go to one XCD, so that
    // they find the slice in that XCD's L2 (the grid is a multiple of 8; items beyond n_items do nothing)
    const int item = (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8);
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
    // i8, b1: the scales of this lane's 16 queries
    [[maybe_unused]] float qs[16];
    if constexpr (I8 || B1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
            qs[r] = q < nqv ? a.qscale[q0 + q] : 0.f;
        }
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
            const T *rp = row_ptr<T>(a.rows, (size_t)(rok ? row : r0), a.dpad);
            if constexpr (B1) {
                i32x16 dot = {};
                ScoreBlock<T>::run(qp, rp, qok, rok, a.dpad, h, dot);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = (float)dot[r] * qs[r];
            } else if constexpr (I8) {
                const float rs = a.rscale[rok ? row : r0];
                i32x16 dot = {};
                ScoreBlock<T>::run(qp, rp, qok, rok, a.dpad, h, dot);
                // (two multiplies in this order and no add: nothing the compiler could contract)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = ((float)dot[r] * qs[r]) * rs;
            } else {
                ScoreBlock<T>::run(qp, rp, qok, rok, a.dpad, h, acc);
            }
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

struct MergeArgs {
    const float *ws_s;                   // [nq][n_cand]
    const int *ws_i;
    int n_cand, k, L;
    int32_t *ids;                        // [nq][k]
    float *scores;
};

// LDS: float scores [L], int ids [L], int count
__global__ __launch_bounds__(NT) void topk_merge_kernel(MergeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int L = a.L, k = a.k, tid = threadIdx.x;
    float *ls = (float *)smem;
    int *li = (int *)(ls + L);
    int *cnt = li + L;
    const float *cs = a.ws_s + (size_t)blockIdx.x * a.n_cand;
    const int *ci = a.ws_i + (size_t)blockIdx.x * a.n_cand;
    for (int i = tid; i < L; i += NT) { ls[i] = -INFINITY; li[i] = SENT_ID; }
    if (tid == 0) *cnt = 0;
    float ts = -INFINITY;
    int ti = SENT_ID;
    __syncthreads();
    const int room = L - k - NT;                 // a round pushes at most NT entries
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
            if (better(s[u], id[u], ts, ti)) {
                const int p = atomicAdd(cnt, 1);
                ls[k + p] = s[u];
                li[k + p] = id[u];
            }
            __syncthreads();
            // (one thread reads the count between the two barriers: the next round's pushes come after the second)
            if (__syncthreads_or(tid == 0 && *cnt > room)) {
                bitonic_sort_lists(ls, li, 1, L, tid);
                ts = ls[k - 1];
                ti = li[k - 1];
                if (tid == 0) *cnt = 0;
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (__syncthreads_or(tid == 0 && *cnt > 0)) bitonic_sort_lists(ls, li, 1, L, tid);
    for (int j = tid; j < k; j += NT) {
        const int id = li[j];
        a.ids[(size_t)blockIdx.x * k + j] = id == SENT_ID ? -1 : id;
        a.scores[(size_t)blockIdx.x * k + j] = ls[j];
    }
}

struct RescoreArgs {
    const void *rows, *queries;          // as TopkArgs
    const float *qscale, *rscale;        // i8: both, b1: qscale
    const uint32_t *live;                // null = every row live
    const int32_t *cand;                 // [nq][n_cand] ids; outside [0, n_rows) = no candidate
    float *ws_s;                         // [nq][n_cand]
    int *ws_i;
    int n_rows, dpad, nq, n_cand, n_blocks;      // n_blocks = ceil(n_cand / 32)
};

// One wave per (query, block of 32 of its candidates): the block's rows are the MFMA's 32 rows, the query is query 0 of the
// tile (the other 31 are zero operands), so lane l < 32 ends with acc[0] = its row's score — the accumulation chain of a search.
template <class T>
__global__ __launch_bounds__(NT) void index_rescore_kernel(RescoreArgs a) {
    constexpr bool I8 = std::is_same_v<T, int8_t>, B1 = std::is_same_v<T, b1_t>;
    using QE = typename QueryElem<T>::type;
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
        const T *rp = row_ptr<T>(a.rows, (size_t)(rok ? id : 0), a.dpad);
        if constexpr (B1) {
            i32x16 dot = {};
            ScoreBlock<T>::run(qp, rp, qok, rok, a.dpad, h, dot);
            s = (float)dot[0] * a.qscale[q];
        } else if constexpr (I8) {
            const float rs = rok ? a.rscale[id] : 0.f;
            i32x16 dot = {};
            ScoreBlock<T>::run(qp, rp, qok, rok, a.dpad, h, dot);
            s = ((float)dot[0] * a.qscale[q]) * rs;            // (the search's two multiplies)
        } else {
            f32x16 acc = {};
            ScoreBlock<T>::run(qp, rp, qok, rok, a.dpad, h, acc);
            s = acc[0];
        }
    }
    if (h == 0 && c < a.n_cand) {
        a.ws_s[(size_t)q * a.n_cand + c] = rok ? s : -INFINITY;
        a.ws_i[(size_t)q * a.n_cand + c] = rok ? id : SENT_ID;
    }
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

template <class T>
void launch_convert(const float *src, void *dst, int n, int dim, int dpad, hipStream_t s) {
    const size_t total = (size_t)n * dpad;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    BERT_LAUNCH(index_convert_kernel<T>, dim3(blocks), dim3(256), 0, s, src, (T *)dst, n, dim, dpad);
}

// f32 rows [n][dim] -> i8 codes [n][dpad] and scales [n] (the i8 form above).  One wave per row: the finite test and the
// maximum of |x_i| across the wave (a maximum is exact in any lane order), then four codes per lane and 32-bit store.
// dpad is a multiple of 32; the division is IEEE (correctly rounded), rint rounds to nearest even.
__global__ __launch_bounds__(256) void index_quantize_kernel(const float *__restrict__ src, int8_t *__restrict__ codes,
                                                             float *__restrict__ scales, int n, int dim, int dpad) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)n) return;                                // (the whole wave)
    const float *x = src + r * dim;
    float amax = 0.f;
    int bad = 0;
    for (int c = lane; c < dim; c += 64) {
        const float v = x[c];
        bad |= !__builtin_isfinite(v);                         // (fmaxf drops a NaN: tested on its own)
        amax = fmaxf(amax, fabsf(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    bad = __any(bad);
    const float scale = bad ? __builtin_nanf("") : amax / 127.0f;
    const bool zero = bad || scale == 0.f;
    if (lane == 0) scales[r] = scale;
    int8_t *out = codes + r * dpad;
    for (int c = 4 * lane; c < dpad; c += 256) {
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = c + j < dim ? x[c + j] : 0.f;
            const float q = zero ? 0.f : fminf(fmaxf(__builtin_rintf(v / scale), -127.f), 127.f);
            packed |= (uint32_t)(uint8_t)(int8_t)(int)q << (8 * j);
        }
        *(uint32_t *)(out + c) = packed;
    }
}

void launch_quantize(const float *src, void *codes, float *scales, int n, int dim, int dpad, hipStream_t s) {
    BERT_LAUNCH(index_quantize_kernel, dim3((n + 3) / 4), dim3(256), 0, s, src, (int8_t *)codes, scales, n, dim, dpad);
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

void launch_pack_b1(const float *src, void *dst, int n, int dim, int dpad, hipStream_t s) {
    BERT_LAUNCH(index_pack_b1_kernel, dim3((n + 3) / 4), dim3(256), 0, s, src, (uint32_t *)dst, n, dim, dpad);
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

// the same on the host mirror
void live_set_range_host(std::vector<uint32_t> &live, int first, int n) {
    for (long long r = first; r < (long long)first + n;) {
        const size_t w = (size_t)(r >> 5);
        const int b = (int)(r & 31);
        const int c = (int)std::min<long long>(32 - b, (long long)first + n - r);
        live[w] |= (c == 32 ? ~0u : ((1u << c) - 1u) << b);
        r += c;
    }
}

size_t live_words(long long rows) { return (size_t)((rows + 31) / 32); }

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(d);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int merge_L(int k) { return k + NT <= 256 ? 256 : 512; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
Index::Plan Index::plan(int n_rows, int nq, int k) {
    Plan p;
    p.nqt = (nq + QT - 1) / QT;
    // slices: enough workgroups to fill the chip, but each slice long against k (the first k rows of a slice all enter its
    // list, and the merge reads slices x k candidates per query)
    const int min_rows = std::max(2048, 16 * k);
    const int s = std::max(1, std::min((TARGET_BLOCKS + p.nqt - 1) / p.nqt, n_rows / min_rows));
    const int per = (int)(((long long)n_rows + s - 1) / s);
    p.slice_rows = std::max(STEP_ROWS, (per + STEP_ROWS - 1) / STEP_ROWS * STEP_ROWS);
    p.slices = std::max(1, (int)(((long long)n_rows + p.slice_rows - 1) / p.slice_rows));
    p.L = k + STEP_ROWS <= 256 ? 256 : 512;
    p.lds = (size_t)std::min(QT, nq) * p.L * 8 + QT * 4;
    return p;
}

size_t Index::ws_entries_bound(int n_rows, int nq, int k) {
    // (plan's slice count is at most this s, which grows with n_rows; taken over every tile count and k' <= k by reserve)
    const int nqt = (nq + QT - 1) / QT, min_rows = std::max(2048, 16 * k);
    const int s = std::max(1, std::min((TARGET_BLOCKS + nqt - 1) / nqt, n_rows / min_rows));
    return (size_t)nq * s * k;
}

Index *Index::create(Engine *eng, int dim, int dtype, std::string &err) {
    if (!eng) { err = "no device engine"; return nullptr; }
    if (dim < 1 || dim > MAX_DIM) { err = "dim must be 1 .. 2048"; return nullptr; }
    if (dtype < 0 || dtype > 3) { err = "dtype must be 0 (f32), 1 (f16), 2 (i8) or 3 (b1)"; return nullptr; }
    DeviceGuard g(eng->device());
    Index *ix = new Index;
    ix->eng_ = eng;
    ix->dim_ = dim;
    ix->dtype_ = dtype;
    // the score kernel's k-step (a 16-byte load per lane)
    ix->dpad_ = index_dpad(dtype, dim);
    ix->row_bytes_ = (size_t)index_row_bytes(dtype, ix->dpad_);
    ix->qrow_bytes_ = dtype == 3 ? (size_t)ix->dpad_ : ix->row_bytes_;      // (b1: the queries are i8 codes)
    const bool ok = hipStreamCreateWithFlags(&ix->stream_, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&ix->busy_, hipEventDisableTiming) == hipSuccess;
    if (!ok) { err = "hipStreamCreate / hipEventCreate failed"; delete ix; return nullptr; }
    // (32 queries x 512-entry lists: 128 KiB of LDS, beyond the 64 KiB a launch gets unasked; a launch that still cannot
    // have it fails, and the search reports the launch error)
    const int lds_max = QT * 512 * 8 + QT * 4;
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<half_t, TopkArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<float, TopkArgs>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<int8_t, TopkArgsI8>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<half_t, TopkArgsMasked>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<float, TopkArgsMasked>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<int8_t, TopkArgsI8Masked>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<b1_t, TopkArgsB1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)index_topk_kernel<b1_t, TopkArgsB1Masked>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    return ix;
}

Index::~Index() {
    DeviceGuard g(eng_ ? eng_->device() : 0);
    if (busy_) { (void)hipEventSynchronize(busy_); (void)hipEventDestroy(busy_); }
    if (stream_) { (void)hipStreamSynchronize(stream_); (void)hipStreamDestroy(stream_); }
    if (rows_) (void)hipFree(rows_);
    if (rscale_) (void)hipFree(rscale_);
    if (live_) (void)hipFree(live_);
}

bool Index::grow(DevBuf &b, size_t bytes, std::string &err) {
    if (bytes <= b.bytes) return true;
    HIP_OK(hipEventSynchronize(busy_), err, false);          // (what is queued may still read the old buffer)
    return b.ensure(bytes, err);
}

bool Index::grow_rows(int n_rows, std::string &err) {
    if (n_rows <= cap_) return true;
    const int cap = (int)std::min<long long>(INT_MAX, std::max<long long>({(long long)n_rows, (long long)cap_ * 3 / 2, 1024}));
    const size_t row_bytes = row_bytes_;
    void *p = nullptr;
    float *sc = nullptr;
    HIP_OK(hipEventSynchronize(busy_), err, false);
    HIP_OK(hipMalloc(&p, (size_t)cap * row_bytes), err, false);
    if (dtype_ == 2 && hipMalloc(&sc, (size_t)cap * 4) != hipSuccess) {
        (void)hipFree(p);
        err = "hipMalloc (index row scales) failed";
        return false;
    }
    // (an index with removed rows: the live words grow with the rows, so that an add within the capacity never allocates)
    uint32_t *lv = nullptr;
    const size_t lw = live_words(cap);
    const char *failed = nullptr;
    if (live_ && hipMalloc(&lv, lw * 4) != hipSuccess) failed = "hipMalloc (index live words) failed";
    else if (n_ > 0 && hipMemcpy(p, rows_, (size_t)n_ * row_bytes, hipMemcpyDeviceToDevice) != hipSuccess) failed = "hipMemcpy (index rows) failed";
    else if (n_ > 0 && sc && hipMemcpy(sc, rscale_, (size_t)n_ * 4, hipMemcpyDeviceToDevice) != hipSuccess) failed = "hipMemcpy (index row scales) failed";
    else if (lv && (hipMemset(lv, 0, lw * 4) != hipSuccess ||
                    hipMemcpy(lv, live_h_.data(), live_words(n_) * 4, hipMemcpyHostToDevice) != hipSuccess)) failed = "hipMemcpy (index live words) failed";
    if (failed) {
        (void)hipFree(p);
        if (sc) (void)hipFree(sc);
        if (lv) (void)hipFree(lv);
        err = failed;
        return false;
    }
    if (rows_) (void)hipFree(rows_);
    if (rscale_) (void)hipFree(rscale_);
    if (live_) { (void)hipFree(live_); live_h_.resize(lw, 0u); }
    rows_ = p;
    rscale_ = sc;
    live_ = lv;
    cap_ = cap;
    return true;
}

bool Index::reserve(int n_rows, int n_queries, int k, std::string &err) {
    if (n_rows < 0 || n_queries < 0 || k < 1 || k > MAX_K) { err = "reserve: n_rows, n_queries >= 0 and 1 <= k <= 256 required"; return false; }
    DeviceGuard g(eng_->device());
    if (!grow_rows(n_rows, err)) return false;
    const int nqc = std::min(n_queries, QCHUNK);
    if (nqc == 0) return true;
    size_t ent = 0;
    const int rows = std::max(n_rows, n_);
    for (int kk = 1; kk <= k; ++kk)
        for (int t = 1; t <= (nqc + QT - 1) / QT; ++t) ent = std::max(ent, ws_entries_bound(rows, std::min(nqc, t * QT), kk));
    return grow(ws_s_, ent * 4, err) && grow(ws_i_, ent * 4, err) && grow_queries(nqc, err);
}

// the stored form of a chunk of nqc queries (i8, b1: codes and scales)
bool Index::grow_queries(int nqc, std::string &err) {
    return grow(qbuf_, (size_t)nqc * qrow_bytes_, err) && (dtype_ < 2 || grow(qscale_, (size_t)nqc * 4, err));
}

int Index::add_device(int n, const float *d_rows, hipStream_t s, std::string &err) {
    if (n < 0 || (n > 0 && !d_rows)) { err = "add: n >= 0 and a row pointer required"; return -1; }
    if ((long long)n_ + n > INT_MAX) { err = "add: an index holds at most 2^31 - 1 rows"; return -1; }
    if (n == 0) return n_;
    DeviceGuard g(eng_->device());
    if (!grow_rows(n_ + n, err)) return -1;
    HIP_OK(hipStreamWaitEvent(s, busy_, 0), err, -1);
    char *dst = (char *)rows_ + (size_t)n_ * row_bytes_;
    eng_->timed_launch(dtype_ == 3 ? "index_pack_b1" : dtype_ == 2 ? "index_quantize_i8" : dtype_ == 1 ? "index_convert_f16" : "index_convert_f32", 0.0, s, [&] {
        if (dtype_ == 3) launch_pack_b1(d_rows, dst, n, dim_, dpad_, s);
        else if (dtype_ == 2) launch_quantize(d_rows, dst, rscale_ + n_, n, dim_, dpad_, s);
        else if (dtype_ == 1) launch_convert<half_t>(d_rows, dst, n, dim_, dpad_, s);
        else launch_convert<float>(d_rows, dst, n, dim_, dpad_, s);
    });
    // (rows added after a removal are live: their bits on the same stream, and in the mirror, which is already long enough)
    if (live_) {
        const int words = (int)(((long long)n_ + n - 1) >> 5) - (n_ >> 5) + 1;
        BERT_LAUNCH(live_set_range_kernel, dim3((words + 255) / 256), dim3(256), 0, s, live_, n_, n);
    }
    HIP_OK(hipGetLastError(), err, -1);
    HIP_OK(hipEventRecord(busy_, s), err, -1);
    if (live_) live_set_range_host(live_h_, n_, n);
    const int first = n_;
    n_ += n;
    return first;
}

int Index::add_host(int n, const float *rows, std::string &err) {
    if (n < 0 || (n > 0 && !rows)) { err = "add: n >= 0 and a row pointer required"; return -1; }
    if ((long long)n_ + n > INT_MAX) { err = "add: an index holds at most 2^31 - 1 rows"; return -1; }
    if (n == 0) return n_;
    DeviceGuard g(eng_->device());
    const int first = n_;
    if (!grow_rows(n_ + n, err)) return -1;
    // through a staging buffer of at most 64 MiB (a row's stored form does not depend on the parts it came in)
    const int per = (int)std::max<size_t>(1, ((size_t)64 << 20) / ((size_t)dim_ * 4));
    for (int i0 = 0; i0 < n; i0 += per) {
        const int c = std::min(per, n - i0);
        if (!grow(stage_, (size_t)c * dim_ * 4, err) ||
            hipMemcpyAsync(stage_.p, rows + (size_t)i0 * dim_, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            add_device(c, stage_.as<float>(), stream_, err) < 0 || hipStreamSynchronize(stream_) != hipSuccess) {
            (void)hipStreamSynchronize(stream_);
            if (err.empty()) err = "add: copy to the device failed";
            truncate(first);
            return -1;
        }
    }
    return first;
}

// f32 queries -> qbuf_ (and qscale_) in the form the score block reads (b1: i8 codes padded to this dpad, and their scales)
void Index::enqueue_queries(int nq, const float *d_q, hipStream_t s) {
    eng_->timed_launch(dtype_ >= 2 ? "index_quantize_i8" : dtype_ == 1 ? "index_convert_f16" : "index_convert_f32", 0.0, s, [&] {
        if (dtype_ >= 2) launch_quantize(d_q, qbuf_.p, qscale_.as<float>(), nq, dim_, dpad_, s);
        else if (dtype_ == 1) launch_convert<half_t>(d_q, qbuf_.p, nq, dim_, dpad_, s);
        else launch_convert<float>(d_q, qbuf_.p, nq, dim_, dpad_, s);
    });
}

void Index::enqueue_chunk(int nq, const float *d_q, int k, int32_t *d_ids, float *d_scores, hipStream_t s, const uint32_t *d_allow) {
    const Plan p = plan(n_, nq, k);
    enqueue_queries(nq, d_q, s);
    TopkArgs a;
    a.rows = rows_; a.queries = qbuf_.p; a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
    a.n_rows = n_; a.dpad = dpad_; a.nq = nq; a.n_qtiles = p.nqt; a.n_slices = p.slices; a.slice_rows = p.slice_rows;
    a.k = k; a.L = p.L; a.n_items = p.nqt * p.slices;
    TopkArgsI8 a8;
    static_cast<TopkArgs &>(a8) = a;
    a8.qscale = qscale_.as<float>(); a8.rscale = rscale_;
    TopkArgsB1 a1;
    static_cast<TopkArgs &>(a1) = a;
    a1.qscale = qscale_.as<float>();
    const int grid = (a.n_items + 7) / 8 * 8;
    const double flops = 2.0 * nq * (double)n_ * dim_;
    if (!live_ && !d_allow) {
        eng_->timed_launch(dtype_ == 3 ? "index_topk_b1" : dtype_ == 2 ? "index_topk_i8" : dtype_ == 1 ? "index_topk_f16" : "index_topk_f32", flops, s, [&] {
            if (dtype_ == 3) BERT_LAUNCH((index_topk_kernel<b1_t, TopkArgsB1>), dim3(grid), dim3(NT), p.lds, s, a1);
            else if (dtype_ == 2) BERT_LAUNCH((index_topk_kernel<int8_t, TopkArgsI8>), dim3(grid), dim3(NT), p.lds, s, a8);
            else if (dtype_ == 1) BERT_LAUNCH((index_topk_kernel<half_t, TopkArgs>), dim3(grid), dim3(NT), p.lds, s, a);
            else BERT_LAUNCH((index_topk_kernel<float, TopkArgs>), dim3(grid), dim3(NT), p.lds, s, a);
        });
    } else {
        // removed rows or an allow-list: the masked kernels, the same plan and workspace
        TopkArgsMasked am;
        static_cast<TopkArgs &>(am) = a;
        am.live = live_; am.allow = d_allow;
        TopkArgsI8Masked am8;
        static_cast<TopkArgsI8 &>(am8) = a8;
        am8.live = live_; am8.allow = d_allow;
        TopkArgsB1Masked am1;
        static_cast<TopkArgsB1 &>(am1) = a1;
        am1.live = live_; am1.allow = d_allow;
        eng_->timed_launch(dtype_ == 3 ? "index_topk_b1_masked" : dtype_ == 2 ? "index_topk_i8_masked" : dtype_ == 1 ? "index_topk_f16_masked" : "index_topk_f32_masked", flops, s, [&] {
            if (dtype_ == 3) BERT_LAUNCH((index_topk_kernel<b1_t, TopkArgsB1Masked>), dim3(grid), dim3(NT), p.lds, s, am1);
            else if (dtype_ == 2) BERT_LAUNCH((index_topk_kernel<int8_t, TopkArgsI8Masked>), dim3(grid), dim3(NT), p.lds, s, am8);
            else if (dtype_ == 1) BERT_LAUNCH((index_topk_kernel<half_t, TopkArgsMasked>), dim3(grid), dim3(NT), p.lds, s, am);
            else BERT_LAUNCH((index_topk_kernel<float, TopkArgsMasked>), dim3(grid), dim3(NT), p.lds, s, am);
        });
    }
    MergeArgs m;
    m.ws_s = a.ws_s; m.ws_i = a.ws_i; m.n_cand = p.slices * k; m.k = k; m.L = merge_L(k); m.ids = d_ids; m.scores = d_scores;
    const size_t lds = (size_t)m.L * 8 + 16;
    eng_->timed_launch("topk_merge", 0.0, s, [&] { BERT_LAUNCH(topk_merge_kernel, dim3(nq), dim3(NT), lds, s, m); });
}

int Index::search_device(int nq, const float *d_q, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                         const uint32_t *d_allow) {
    if (k < 1 || k > MAX_K) { err = "search: k must be 1 .. 256"; return -1; }
    if (nq < 0 || (nq > 0 && (!d_q || !d_ids || !d_scores))) { err = "search: n_queries >= 0 and query / result pointers required"; return -1; }
    if (nq == 0) return 0;
    DeviceGuard g(eng_->device());
    const int nqc = std::min(nq, QCHUNK);
    // (the last, shorter chunk may be cut into more slices than a full one)
    const size_t ent = std::max(ws_entries_bound(n_, nqc, k), nq % QCHUNK ? ws_entries_bound(n_, nq % QCHUNK, k) : 0);
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow_queries(nqc, err)) return -1;
    HIP_OK(hipStreamWaitEvent(s, busy_, 0), err, -1);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        enqueue_chunk(c, d_q + (size_t)c0 * dim_, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s, d_allow);
    }
    HIP_OK(hipGetLastError(), err, -1);
    HIP_OK(hipEventRecord(busy_, s), err, -1);
    return 0;
}

int Index::search_to_host(int nq, const float *q, bool q_on_device, int k, int32_t *ids, float *scores, std::string &err,
                          const uint32_t *allow) {
    if (k < 1 || k > MAX_K) { err = "search: k must be 1 .. 256"; return -1; }
    if (nq < 0 || (nq > 0 && (!q || !ids || !scores))) { err = "search: n_queries >= 0 and query / result pointers required"; return -1; }
    if (nq == 0) return 0;
    DeviceGuard g(eng_->device());
    std::vector<int32_t> hid((size_t)nq * k);
    std::vector<float> hsc((size_t)nq * k);
    const uint32_t *d_allow = nullptr;
    if (allow && n_ > 0) {
        // (the first search below waits for this copy: the same stream)
        if (!grow(allow_, live_words(n_) * 4, err)) return -1;
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -1);
        HIP_OK(hipMemcpyAsync(allow_.p, allow, live_words(n_) * 4, hipMemcpyHostToDevice, stream_), err, -1);
        d_allow = allow_.as<uint32_t>();
    }
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const float *dq = q + (size_t)c0 * dim_;
        if (!q_on_device) {
            if (!grow(stage_, (size_t)c * dim_ * 4, err)) return -1;
            HIP_OK(hipMemcpyAsync(stage_.p, dq, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_), err, -1);
            dq = stage_.as<float>();
        }
        if (!grow(out_ids_, (size_t)c * k * 4, err) || !grow(out_scores_, (size_t)c * k * 4, err)) return -1;
        if (search_device(c, dq, k, out_ids_.as<int32_t>(), out_scores_.as<float>(), stream_, err, d_allow) != 0) { (void)hipStreamSynchronize(stream_); return -1; }
        HIP_OK(hipMemcpyAsync(hid.data() + (size_t)c0 * k, out_ids_.p, (size_t)c * k * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipMemcpyAsync(hsc.data() + (size_t)c0 * k, out_scores_.p, (size_t)c * k * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
    }
    memcpy(ids, hid.data(), hid.size() * 4);
    memcpy(scores, hsc.data(), hsc.size() * 4);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// rescoring, two-stage search
// ------------------------------------------------------------------------------------------------
int Index::rescore_device(int nq, const float *d_q, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids, float *d_scores,
                          hipStream_t s, std::string &err) {
    if (k < 1 || k > MAX_K) { err = "rescore: k must be 1 .. 256"; return -1; }
    if (n_cand < 1 || n_cand > MAX_CAND) { err = "rescore: n_cand must be 1 .. 1024"; return -1; }
    if (nq < 0 || (nq > 0 && (!d_q || !d_cand || !d_ids || !d_scores))) { err = "rescore: n_queries >= 0 and query / candidate / result pointers required"; return -1; }
    if (nq == 0) return 0;
    DeviceGuard g(eng_->device());
    const int nqc = std::min(nq, QCHUNK);
    const size_t ent = (size_t)nqc * n_cand;
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow_queries(nqc, err)) return -1;
    HIP_OK(hipStreamWaitEvent(s, busy_, 0), err, -1);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        enqueue_queries(c, d_q + (size_t)c0 * dim_, s);
        RescoreArgs a;
        a.rows = rows_; a.queries = qbuf_.p; a.qscale = qscale_.as<float>(); a.rscale = rscale_; a.live = live_;
        a.cand = d_cand + (size_t)c0 * n_cand; a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
        a.n_rows = n_; a.dpad = dpad_; a.nq = c; a.n_cand = n_cand; a.n_blocks = (n_cand + 31) / 32;
        const int grid = (c * a.n_blocks + NWAVE - 1) / NWAVE;
        const double flops = 2.0 * c * (double)n_cand * dim_;
        eng_->timed_launch(dtype_ == 3 ? "index_rescore_b1" : dtype_ == 2 ? "index_rescore_i8" : dtype_ == 1 ? "index_rescore_f16" : "index_rescore_f32", flops, s, [&] {
            if (dtype_ == 3) BERT_LAUNCH(index_rescore_kernel<b1_t>, dim3(grid), dim3(NT), 0, s, a);
            else if (dtype_ == 2) BERT_LAUNCH(index_rescore_kernel<int8_t>, dim3(grid), dim3(NT), 0, s, a);
            else if (dtype_ == 1) BERT_LAUNCH(index_rescore_kernel<half_t>, dim3(grid), dim3(NT), 0, s, a);
            else BERT_LAUNCH(index_rescore_kernel<float>, dim3(grid), dim3(NT), 0, s, a);
        });
        MergeArgs m;
        m.ws_s = a.ws_s; m.ws_i = a.ws_i; m.n_cand = n_cand; m.k = k; m.L = merge_L(k);
        m.ids = d_ids + (size_t)c0 * k; m.scores = d_scores + (size_t)c0 * k;
        const size_t lds = (size_t)m.L * 8 + 16;
        eng_->timed_launch("topk_merge", 0.0, s, [&] { BERT_LAUNCH(topk_merge_kernel, dim3(c), dim3(NT), lds, s, m); });
    }
    HIP_OK(hipGetLastError(), err, -1);
    HIP_OK(hipEventRecord(busy_, s), err, -1);
    return 0;
}

int Index::rescore_to_host(int nq, const float *q, int n_cand, const int32_t *cand, int k, int32_t *ids, float *scores, std::string &err) {
    if (k < 1 || k > MAX_K) { err = "rescore: k must be 1 .. 256"; return -1; }
    if (n_cand < 1 || n_cand > MAX_CAND) { err = "rescore: n_cand must be 1 .. 1024"; return -1; }
    if (nq < 0 || (nq > 0 && (!q || !cand || !ids || !scores))) { err = "rescore: n_queries >= 0 and query / candidate / result pointers required"; return -1; }
    if (nq == 0) return 0;
    DeviceGuard g(eng_->device());
    std::vector<int32_t> hid((size_t)nq * k);
    std::vector<float> hsc((size_t)nq * k);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        if (!grow(stage_, (size_t)c * dim_ * 4, err) || !grow(cand_in_, (size_t)c * n_cand * 4, err) ||
            !grow(out_ids_, (size_t)c * k * 4, err) || !grow(out_scores_, (size_t)c * k * 4, err))
            return -1;
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -1);
        HIP_OK(hipMemcpyAsync(stage_.p, q + (size_t)c0 * dim_, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_), err, -1);
        HIP_OK(hipMemcpyAsync(cand_in_.p, cand + (size_t)c0 * n_cand, (size_t)c * n_cand * 4, hipMemcpyHostToDevice, stream_), err, -1);
        if (rescore_device(c, stage_.as<float>(), n_cand, cand_in_.as<int32_t>(), k, out_ids_.as<int32_t>(), out_scores_.as<float>(), stream_, err) != 0) {
            (void)hipStreamSynchronize(stream_);
            return -1;
        }
        HIP_OK(hipMemcpyAsync(hid.data() + (size_t)c0 * k, out_ids_.p, (size_t)c * k * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipMemcpyAsync(hsc.data() + (size_t)c0 * k, out_scores_.p, (size_t)c * k * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
    }
    memcpy(ids, hid.data(), hid.size() * 4);
    memcpy(scores, hsc.data(), hsc.size() * 4);
    return 0;
}

int Index::search_rescored_device(Index &coarse, int nq, const float *d_q, int n_cand, int k, int32_t *d_ids, float *d_scores,
                                  hipStream_t s, std::string &err) {
    if (n_cand < 1 || n_cand > MAX_K || k < 1 || k > n_cand) { err = "search_rescored: 1 <= k <= n_cand <= 256 required"; return -1; }
    if (nq < 0 || (nq > 0 && (!d_q || !d_ids || !d_scores))) { err = "search_rescored: n_queries >= 0 and query / result pointers required"; return -1; }
    if (nq == 0) return 0;
    DeviceGuard g(eng_->device());
    const int nqc = std::min(nq, QCHUNK);
    if (!grow(cand_i_, (size_t)nqc * n_cand * 4, err) || !grow(cand_s_, (size_t)nqc * n_cand * 4, err)) return -1;
    // (the candidate lists are this index's: the coarse search that fills them waits for whatever still reads them; after
    // that the two steps of a chunk, and the chunks, follow each other on s)
    HIP_OK(hipStreamWaitEvent(s, busy_, 0), err, -1);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const float *dq = d_q + (size_t)c0 * dim_;
        if (coarse.search_device(c, dq, n_cand, cand_i_.as<int32_t>(), cand_s_.as<float>(), s, err) != 0) return -1;
        if (rescore_device(c, dq, n_cand, cand_i_.as<int32_t>(), k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s, err) != 0) return -1;
    }
    return 0;
}

int Index::search_rescored_to_host(Index &coarse, int nq, const float *q, int n_cand, int k, int32_t *ids, float *scores, std::string &err) {
    if (n_cand < 1 || n_cand > MAX_K || k < 1 || k > n_cand) { err = "search_rescored: 1 <= k <= n_cand <= 256 required"; return -1; }
    if (nq < 0 || (nq > 0 && (!q || !ids || !scores))) { err = "search_rescored: n_queries >= 0 and query / result pointers required"; return -1; }
    if (nq == 0) return 0;
    DeviceGuard g(eng_->device());
    std::vector<int32_t> hid((size_t)nq * k);
    std::vector<float> hsc((size_t)nq * k);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        if (!grow(stage_, (size_t)c * dim_ * 4, err) || !grow(out_ids_, (size_t)c * k * 4, err) || !grow(out_scores_, (size_t)c * k * 4, err)) return -1;
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -1);
        HIP_OK(hipMemcpyAsync(stage_.p, q + (size_t)c0 * dim_, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_), err, -1);
        if (search_rescored_device(coarse, c, stage_.as<float>(), n_cand, k, out_ids_.as<int32_t>(), out_scores_.as<float>(), stream_, err) != 0) {
            (void)hipStreamSynchronize(stream_);
            return -1;
        }
        HIP_OK(hipMemcpyAsync(hid.data() + (size_t)c0 * k, out_ids_.p, (size_t)c * k * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipMemcpyAsync(hsc.data() + (size_t)c0 * k, out_scores_.p, (size_t)c * k * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
    }
    memcpy(ids, hid.data(), hid.size() * 4);
    memcpy(scores, hsc.data(), hsc.size() * 4);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// removed rows, compaction, file form
// ------------------------------------------------------------------------------------------------
void Index::truncate(int n) {
    if (n < 0 || n >= n_) return;
    // (the mirror keeps its bits at and beyond size zero; the device words of the dropped rows stay as they are: a search
    // ignores them, and the add that reuses those rows sets them)
    if (live_) {
        for (long long r = n; r < n_;) {
            const int b = (int)(r & 31);
            live_h_[(size_t)(r >> 5)] &= b ? (1u << b) - 1u : 0u;
            r += 32 - b;
        }
        n_removed_ = n;
        for (size_t w = 0; w < live_words(n); ++w) n_removed_ -= __builtin_popcount(live_h_[w]);
    }
    n_ = n;
}

// the bitmap of an index that had none: every row live
bool Index::make_live(std::string &err) {
    if (live_) return true;
    const size_t lw = live_words(cap_);
    HIP_OK(hipEventSynchronize(busy_), err, false);
    HIP_OK(hipMalloc((void **)&live_, std::max<size_t>(lw, 1) * 4), err, false);
    live_h_.assign(lw, 0u);
    if (n_ > 0) live_set_range_host(live_h_, 0, n_);
    n_removed_ = 0;
    if (hipMemcpy(live_, live_h_.data(), lw * 4, hipMemcpyHostToDevice) != hipSuccess) {
        drop_live();
        err = "hipMemcpy (index live words) failed";
        return false;
    }
    return true;
}

void Index::drop_live() {
    if (live_) (void)hipFree(live_);
    live_ = nullptr;
    live_h_.clear();
    n_removed_ = 0;
}

// mirror words [w0, w1) -> device, on the index's stream behind whatever is queued; blocking
bool Index::upload_live(size_t w0, size_t w1, std::string &err) {
    if (w1 <= w0) return true;
    HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, false);
    HIP_OK(hipMemcpyAsync(live_ + w0, live_h_.data() + w0, (w1 - w0) * 4, hipMemcpyHostToDevice, stream_), err, false);
    HIP_OK(hipEventRecord(busy_, stream_), err, false);
    HIP_OK(hipStreamSynchronize(stream_), err, false);
    return true;
}

int Index::remove(int n, const int32_t *ids, std::string &err) {
    if (n < 0 || (n > 0 && !ids)) { err = "remove: n >= 0 and an id pointer required"; return -1; }
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= n_) { err = "remove: id " + std::to_string(ids[i]) + " is outside [0, " + std::to_string(n_) + ")"; return -1; }
    if (n == 0) return 0;
    DeviceGuard g(eng_->device());
    if (!make_live(err)) return -1;
    std::vector<int32_t> fresh;                          // the ids this call removes (repeats and removed rows left out)
    size_t w0 = SIZE_MAX, w1 = 0;
    for (int i = 0; i < n; ++i) {
        const size_t w = (size_t)ids[i] >> 5;
        const uint32_t bit = 1u << (ids[i] & 31);
        if (!(live_h_[w] & bit)) continue;
        live_h_[w] &= ~bit;
        fresh.push_back(ids[i]);
        w0 = std::min(w0, w);
        w1 = std::max(w1, w + 1);
    }
    if (!fresh.empty() && !upload_live(w0, w1, err)) {
        for (int32_t id : fresh) live_h_[(size_t)id >> 5] |= 1u << (id & 31);      // (the mirror as it was)
        return -1;
    }
    n_removed_ += (int)fresh.size();
    return (int)fresh.size();
}

int Index::compact(int32_t *old_ids, std::string &err) {
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -1);
    if (n_removed_ == 0) {
        if (old_ids) for (int i = 0; i < n_; ++i) old_ids[i] = i;
        drop_live();
        return n_;
    }
    const int nl = n_ - n_removed_;
    std::vector<int32_t> map((size_t)nl);
    int j = 0;
    for (int r = 0; r < n_; ++r)
        if (live_h_[(size_t)r >> 5] >> (r & 31) & 1u) map[(size_t)j++] = r;
    const size_t row_bytes = row_bytes_;
    void *p = nullptr;
    float *sc = nullptr;
    int32_t *d_map = nullptr;
    const char *failed = nullptr;
    if (nl > 0) {
        if (hipMalloc(&p, (size_t)nl * row_bytes) != hipSuccess) failed = "hipMalloc (index rows) failed";
        else if (dtype_ == 2 && hipMalloc((void **)&sc, (size_t)nl * 4) != hipSuccess) failed = "hipMalloc (index row scales) failed";
        else if (hipMalloc((void **)&d_map, (size_t)nl * 4) != hipSuccess) failed = "hipMalloc (compaction ids) failed";
        else if (hipMemcpyAsync(d_map, map.data(), (size_t)nl * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) failed = "hipMemcpy (compaction ids) failed";
        else {
            const int pieces = (int)(row_bytes / 16);
            const int blocks = (int)std::min<size_t>(((size_t)nl * pieces + 255) / 256, 16384);
            eng_->timed_launch("index_gather", 0.0, stream_, [&] {
                BERT_LAUNCH(index_gather_kernel, dim3(blocks), dim3(256), 0, stream_, (const i32x4 *)rows_, (i32x4 *)p, rscale_, sc, d_map, nl, pieces);
            });
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) failed = "the gather kernel failed";
        }
        if (d_map) (void)hipFree(d_map);
        if (failed) {
            if (p) (void)hipFree(p);
            if (sc) (void)hipFree(sc);
            err = failed;
            return -1;
        }
    }
    if (rows_) (void)hipFree(rows_);
    if (rscale_) (void)hipFree(rscale_);
    rows_ = p;
    rscale_ = sc;
    cap_ = n_ = nl;
    drop_live();
    if (old_ids) memcpy(old_ids, map.data(), (size_t)nl * 4);
    return nl;
}

namespace {

// device memory <-> file in pieces of at most 64 MiB through a host buffer
constexpr size_t FILE_PIECE = (size_t)64 << 20;

bool device_to_file(FILE *f, const void *d, size_t bytes, std::vector<char> &buf, std::string &err) {
    for (size_t o = 0; o < bytes; o += FILE_PIECE) {
        const size_t c = std::min(FILE_PIECE, bytes - o);
        if (buf.size() < c) buf.resize(c);
        HIP_OK(hipMemcpy(buf.data(), (const char *)d + o, c, hipMemcpyDeviceToHost), err, false);
        if (fwrite(buf.data(), 1, c, f) != c) { err = "write failed"; return false; }
    }
    return true;
}

bool file_to_device(FILE *f, void *d, size_t bytes, std::vector<char> &buf, std::string &err) {
    for (size_t o = 0; o < bytes; o += FILE_PIECE) {
        const size_t c = std::min(FILE_PIECE, bytes - o);
        if (buf.size() < c) buf.resize(c);
        if (fread(buf.data(), 1, c, f) != c) { err = "read failed"; return false; }
        HIP_OK(hipMemcpy((char *)d + o, buf.data(), c, hipMemcpyHostToDevice), err, false);
    }
    return true;
}

}  // namespace

bool Index::save(const char *path, std::string &err) {
    if (!path || !*path) { err = "a path is required"; return false; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, false);
    IndexFileHeader h;
    h.dtype = (uint32_t)dtype_; h.dim = (uint32_t)dim_; h.dpad = (uint32_t)dpad_; h.n_rows = (uint32_t)n_; h.has_live = live_ ? 1u : 0u;
    unsigned char hdr[INDEX_HEADER_BYTES];
    index_header_write(h, hdr);
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) { err = "cannot write '" + tmp + "'"; return false; }
    std::vector<char> buf;
    // (the live words come from the mirror: its bits at and beyond size are zero)
    bool ok = fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr && device_to_file(f, rows_, (size_t)n_ * row_bytes_, buf, err) &&
              (dtype_ != 2 || device_to_file(f, rscale_, (size_t)n_ * 4, buf, err)) &&
              (!live_ || fwrite(live_h_.data(), 4, live_words(n_), f) == live_words(n_));
    ok = (fclose(f) == 0) && ok;
    if (ok && rename(tmp.c_str(), path) != 0) ok = false;
    if (!ok) {
        (void)::remove(tmp.c_str());
        if (err.empty()) err = "cannot write '" + std::string(path) + "'";
    }
    return ok;
}

bool Index::load_rows(FILE *f, const IndexFileHeader &h, std::string &err) {
    if (n_ != 0 || live_ || (int)h.dtype != dtype_ || (int)h.dim != dim_ || (int)h.dpad != dpad_) { err = "load: the index does not fit the file"; return false; }
    DeviceGuard g(eng_->device());
    const int n = (int)h.n_rows;
    if (!grow_rows(n, err)) return false;
    std::vector<char> buf;
    if (!file_to_device(f, rows_, (size_t)n * row_bytes_, buf, err)) return false;
    if (dtype_ == 2 && !file_to_device(f, rscale_, (size_t)n * 4, buf, err)) return false;
    n_ = n;
    if (!h.has_live) return true;
    std::vector<uint32_t> words(live_words(n));
    if (fread(words.data(), 4, words.size(), f) != words.size()) { n_ = 0; err = "read failed"; return false; }
    if (n & 31 && !words.empty() && (words.back() >> (n & 31)) != 0) { n_ = 0; err = "live bits beyond the last row"; return false; }
    if (!make_live(err)) { n_ = 0; return false; }
    std::copy(words.begin(), words.end(), live_h_.begin());
    for (uint32_t w : words) n_removed_ += 32 - __builtin_popcount(w);
    n_removed_ -= (int)(words.size() * 32 - (size_t)n);          // (the last word's bits beyond n are zero, not removed rows)
    if (!upload_live(0, words.size(), err)) { drop_live(); n_ = 0; return false; }
    return true;
}

float *Index::scratch(size_t n, std::string &err) {
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, nullptr);
    return scratch_.ensure(n * 4, err) ? scratch_.as<float>() : nullptr;
}

}  // namespace bert_hip
