// token_index.hip — the device code of the token index (gfx950; bert_hip.h "TOKEN INDEX" and "TOKEN INDEX, int8 form"): documents'
// token rows in HBM — f16 rows, or int8 codes with one f32 scale per token — and their exact MaxSim top-k search.  The kernels and their
// launchers (token_index_kernels.h, which states both stored forms); the TokenIndex class that plans and orders them is token_index.cpp
// (token_index.h).
//
//   token_index_scan_kernel<Form, MASKED, LISTED>  ONE skeleton — the work map, the guards, the list, the step mask, the round loop and
//                   its barriers, the selection, the write-out — stated once; a Form (F16Form, I8Form) holds only how a query is staged in
//                   LDS and how one document is scored.  Five instantiations: f16 plain and masked; int8 plain, masked and listed.
//   Skeleton.       One workgroup of four waves per (query, slice of consecutive documents).  The workgroup stages ALL the query's blocks
//                   of 32 tokens in LDS once (Form::stage).  Then each wave takes whole documents of the slice — first + wave,
//                   first + wave + 4, ... — and scores each alone (Form::score).  No LDS exchange between waves: a document belongs to
//                   one wave, a short one costs one chain and one reduction.
//   Selection.      topk_select.h's queue with one list, the threshold in registers; lane 0 of a wave pushes a document that beats
//                   the threshold; every TOKEN_ROUNDS documents per wave the workgroup looks at the count (select_step_end).  The trip
//                   counts are the workgroup's — a wave without a document in a round scores nothing —, so every barrier is met by all
//                   four waves.  k entries per (query, slice) reach the workspace, which topk_merge_kernel merges; the scores never
//                   reach HBM.
//   Guards.         A query that is empty, descends, starts below 0 or is longer than the launch's max_q_len gets k entries of
//                   (-inf, INT_MAX) in every slice — id -1 / -INFINITY after the merge —; nothing else is touched.  So does a query that
//                   its form calls bad when it stages it (int8: a NaN scale).
//   MASKED.         Removed documents and allow-lists: the same body with a 64-bit mask per step of TOKEN_STEP_DOCS documents, built from
//                   up to three words of live & allow that every wave loads through the scalar path.  A wave skips a document whose bit
//                   is clear before it reads the document's lengths or rows, INSIDE the round loop, so the step's barriers are met by
//                   all four waves whatever each of them scored; a step whose mask is zero is skipped by the whole workgroup, barriers
//                   included (the mask is the workgroup's, and nothing was pushed).  A step still pushes at most TOKEN_STEP_DOCS
//                   entries: L and the room rule are those of the unmasked instantiation, which contains none of this.
//   LISTED.         A rescore (int8 form only; the f16 form's is maxsim_kernel behind token_index_pairs_kernel): a slice is a range of
//                   positions of the query's candidate list, a wave's document id comes from the list; an id outside [0, n_docs) or a
//                   removed one is no candidate, a repeated id is pushed each time.  One wave still sees a whole document: the search's
//                   bits by construction.
//   F16Form.        Query rows of dim + 8 halfs (maxsim's padding: the 32 rows a ds_read_b128 step touches lie on distinct bank groups;
//                   the slots behind the query's end are zero-filled).  Per query block the wave walks the document's 32-token blocks
//                   straight from global memory / L2, runs score_chain_f16 with the document block as the A operand and the query block
//                   as the B operand, keeps the running elementwise max in 16 registers, masks only the document's last block, folds
//                   the 16 maxima, meets lane ^ 32 (xor32_max) and adds the block's 32 maxima with wave_sum_f32 — the expressions of
//                   maxsim_kernel, whose four waves' maxima meet by an exact max where here one wave saw them all.
//                   maxsim's masking: a document slot at or behind the document's end enters the max as -inf (its operand is zero-filled
//                   in registers, never read); a query slot at or behind the query's end adds +0.  No lane reads a row outside
//                   [cu[d], cu[d + 1]) of its document or outside the query's range.
//   I8Form.         v_mfma_i32_32x32x32_i8.
//     Query.        Staged once in LDS: codes as rows of dpad + 16 bytes, the scales beside them.  A ds_read_b128 step reads the 16 bytes
//                   at 32 s + 16 h of row col; its lane groups (MI355X: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) hold 16
//                   rows of all 16 residues mod 16 at one h, the row stride is (dpad / 16 + 1) slots of 16 bytes — an odd number, dpad being a
//                   multiple of 32 —, so the 16 rows lie on the 16 distinct slots of the 256-byte bank row: no conflict.
//     Score.        dot_ij exact in i32 (the document block is the A operand straight from global memory: lane (col, h) feeds step s
//                   the 16 bytes at 32 s + 16 h of row j0 + col — ScoreBlock<int8_t>::run's k map).  acc[r] is document token
//                   j0 + (r & 3) + 8 (r >> 2) + 4 h against query token col: per block of 32 document tokens 16 conversions (exact:
//                   |dot| < 2^24), 16 multiplies by the token's scale and 16 maxima; the 16 scales of a lane are four runs of four
//                   consecutive floats at j0 + 8 g + 4 h, whose alignment nothing promises (a 4-byte aligned 16-byte load).  The maximum
//                   m_i over the document is multiplied ONCE by the query token's scale, and the products are added as the f16 form adds
//                   its maxima: blocks of 32 through wave_sum_f32 with +0 in lanes 32 .. 63 and behind the query's end, the blocks'
//                   sums in ascending order from +0.
//     Non-finite.   fmaxf drops a NaN, so a NaN scale is looked for on its own: a document with one (the unsigned maximum of the scales'
//                   bits is above +inf's) scores nothing and is never pushed; a query with one gets the guards' lists.
//   token_i8_quantize_kernel  f32 or f16 rows (f16 is converted exactly) -> codes and scales, one wave per row by device.h's
//                   quantize_row_i8 — the embedding index's rule, stated there once.  Serves the adds and, with qcu, the queries of every
//                   search and rescore.
//   token_index_pairs_kernel  an f16 rescore's candidate ids as maxsim's pair list (token_index_kernels.h); a removed id is no candidate.
//   token_index_gather_kernel  compaction: the kept documents' rows into a fresh allocation (see the kernel).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "device.h"
#include "score_chain.h"
#include "token_index_kernels.h"
#include "topk_select.h"

namespace bert_hip {

namespace {

static_assert(TOKEN_STEP_DOCS == 64, "the masked scan keeps a step's mask in one 64-bit word");

// the word of live & allow (a null pointer: all ones) at index wi, the same in every lane
__device__ __forceinline__ uint32_t token_mask_word(const TokenScanArgs &a, int wi) {
    uint32_t w = ~0u;
    if (a.live) w &= a.live[wi];
    if (a.allow) w &= a.allow[wi];
    return __builtin_amdgcn_readfirstlane(w);
}

// A Form of token_index_scan_kernel: how the query is staged and how one document is scored.  Its members are a few pointers and a
// row stride, held in registers.
//   init   lays the staged query out at the front of the launch's LDS and returns the first byte behind it (the skeleton's list)
//   stage  query qi's nq tokens (rows q0 ..) into LDS, slots behind its end zero-filled; this thread's part of "the query is bad".
//          The skeleton's barrier follows
//   score  the whole wave: document rows d0 .. d0 + nd - 1 against the staged query, the total the same in every lane; bad: the
//          document must not be pushed (the same in every lane)

struct F16Form {
    static constexpr bool LISTABLE = false;             // (a rescore of f16 rows is maxsim's)
    static constexpr bool BAD_QUERIES = false;          // (stage never says bad: the skeleton's barrier behind it is a plain one)
    static constexpr int PLAIN_PAD = 2;                 // (the skeleton's code placement)
    half_t *qs;                                         // [blocks of the launch][32][ldq]
    int H, ldq;

    __device__ __forceinline__ unsigned char *init(const TokenScanArgs &a, unsigned char *lds) {
        H = a.dim; ldq = H + 8;
        qs = (half_t *)lds;
        return lds + (size_t)((a.max_q_len + TOKEN_QB - 1) / TOKEN_QB) * TOKEN_QB * ldq * 2;
    }
    __device__ __forceinline__ bool stage(const TokenScanArgs &a, int, int q0, int nq, int nblk, int tid) const {
        const int chunks = H >> 3;                      // (chunks: 16-byte pieces of a row)
        const half_t *q = (const half_t *)a.q;
        const f16x8 z = {};
        for (int i = tid; i < nblk * TOKEN_QB * chunks; i += NT) {
            const int r = i / chunks, c = i - r * chunks;
            *(f16x8 *)(qs + r * ldq + 8 * c) = r < nq ? *(const f16x8 *)(q + (size_t)(q0 + r) * H + 8 * c) : z;
        }
        return false;
    }
    __device__ __forceinline__ float score(const TokenScanArgs &a, int d0, int nd, int nq, int nblk, int lane, bool &bad) const {
        const int col = lane & 31, h = lane >> 5;
        const half_t *rows = (const half_t *)a.rows;
        const f16x8 z = {};
        bad = false;
        float total = 0.f;
        for (int qb = 0; qb < nblk; ++qb) {
            const bool qok = qb * TOKEN_QB + col < nq;
            const half_t *qrow = qs + (qb * TOKEN_QB + col) * ldq;
            f32x16 m;
#pragma unroll
            for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
            for (int j0 = 0; j0 < nd; j0 += 32) {
                const bool dok = j0 + col < nd;            // this lane's row of the A operand: document token j0 + col
                const half_t *drow = rows + (size_t)(d0 + (dok ? j0 + col : 0)) * H;
                f32x16 acc = {};
                score_chain_f16([&](int kk, bool in) __attribute__((always_inline)) { return dok && in && kk + 8 * h < H ? *(const f16x8 *)(drow + kk + 8 * h) : z; },
                                [&](int kk, bool in) __attribute__((always_inline)) { return qok && in && kk + 8 * h < H ? *(const f16x8 *)(qrow + kk + 8 * h) : z; },
                                H, acc);
                if (j0 + 32 <= nd) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) m[r] = __builtin_fmaxf(m[r], acc[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        m[r] = __builtin_fmaxf(m[r], j < nd ? acc[r] : -INFINITY);
                    }
                }
            }
            float v = m[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) v = __builtin_fmaxf(v, m[r]);
            v = xor32_max(v);
            total += wave_sum_f32(h == 0 && qok ? v : 0.f);
        }
        return total;
    }
};

// four consecutive scales at any 4-byte aligned address
struct __attribute__((aligned(4))) f32x4u { float v[4]; };

struct I8Form {
    static constexpr bool LISTABLE = true;
    static constexpr bool BAD_QUERIES = true;           // (a query with a non-finite token)
    static constexpr int PLAIN_PAD = 16;
    int8_t *qs;                                         // [blocks of the launch][32][ldq]
    float *qsc;                                         // [TOKEN_MAX_QUERY]
    int P, ldq;

    __device__ __forceinline__ unsigned char *init(const TokenScanArgs &a, unsigned char *lds) {
        P = a.dpad; ldq = P + 16;
        qs = (int8_t *)lds;
        qsc = (float *)(lds + (size_t)((a.max_q_len + TOKEN_QB - 1) / TOKEN_QB) * TOKEN_QB * ldq);
        return (unsigned char *)(qsc + TOKEN_MAX_QUERY);
    }
    __device__ __forceinline__ bool stage(const TokenScanArgs &a, int qi, int, int nq, int nblk, int tid) const {
        const int chunks = P >> 4;                      // (chunks: 16-byte pieces of a row)
        const i32x4 z = {};
        const int8_t *qsrc = (const int8_t *)a.q + (size_t)qi * a.max_q_len * P;
        for (int i = tid; i < nblk * TOKEN_QB * chunks; i += NT) {
            const int r = i / chunks, c = i - r * chunks;
            *(i32x4 *)(qs + r * ldq + 16 * c) = r < nq ? *(const i32x4 *)(qsrc + (size_t)r * P + 16 * c) : z;
        }
        bool qbad = false;
        for (int i = tid; i < nblk * TOKEN_QB; i += NT) {
            const float s = i < nq ? a.q_scales[(size_t)qi * a.max_q_len + i] : 0.f;
            qsc[i] = s;
            qbad |= s != s;
        }
        return qbad;
    }
    __device__ __forceinline__ float score(const TokenScanArgs &a, int d0, int nd, int nq, int nblk, int lane, bool &bad) const {
        const int col = lane & 31, h = lane >> 5;
        const int8_t *codes = (const int8_t *)a.rows;
        const i32x4 z = {};
        float total = 0.f;
        uint32_t sbits = 0;                                // the unsigned maximum of the document's scales' bits
        for (int qb = 0; qb < nblk; ++qb) {
            const bool qok = qb * TOKEN_QB + col < nq;
            const int8_t *qrow = qs + (qb * TOKEN_QB + col) * ldq + 16 * h;
            f32x16 mx;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx[r] = -INFINITY;
            for (int j0 = 0; j0 < nd; j0 += 32) {
                const bool dok = j0 + col < nd;            // this lane's row of the A operand: document token j0 + col
                const bool full = j0 + 32 <= nd;
                const int8_t *drow = codes + (size_t)(d0 + (dok ? j0 + col : 0)) * P + 16 * h;
                const float *sp = a.scales + (size_t)d0 + j0 + 4 * h;
                // the scales of this lane's 16 document tokens (a slot behind the document's end: 0, never read)
                float sc[16];
                if (full) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4u v = *(const f32x4u *)(sp + 8 * g);
                        sc[4 * g] = v.v[0]; sc[4 * g + 1] = v.v[1]; sc[4 * g + 2] = v.v[2]; sc[4 * g + 3] = v.v[3];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int o = (r & 3) + 8 * (r >> 2);
                        sc[r] = j0 + o + 4 * h < nd ? sp[o] : 0.f;
                    }
                }
                i32x16 acc = {};
                constexpr int U = 8;
                for (int k0 = 0; k0 < P; k0 += 32 * U) {
                    i32x4 av[U], bv[U];
#pragma unroll
                    for (int uu = 0; uu < U; ++uu) {
                        const bool in = k0 + 32 * uu < P;
                        av[uu] = dok && in ? *(const i32x4 *)(drow + k0 + 32 * uu) : z;
                        bv[uu] = qok && in ? *(const i32x4 *)(qrow + k0 + 32 * uu) : z;
                    }
#pragma unroll
                    for (int uu = 0; uu < U; ++uu)
                        if (k0 + 32 * uu < P) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[uu], bv[uu], acc, 0, 0, 0);
                }
                if (qb == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) sbits = max(sbits, __builtin_bit_cast(uint32_t, sc[r]));
                }
                if (full) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx[r] = __builtin_fmaxf(mx[r], (float)acc[r] * sc[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        mx[r] = __builtin_fmaxf(mx[r], j < nd ? (float)acc[r] * sc[r] : -INFINITY);
                    }
                }
            }
            float v = mx[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) v = __builtin_fmaxf(v, mx[r]);
            v = xor32_max(v);
            // (one multiply by the query token's scale, behind the max; rounded_f32: a product of its own, never fused into the sum)
            total += wave_sum_f32(h == 0 && qok ? rounded_f32(v * qsc[qb * TOKEN_QB + col]) : 0.f);
        }
        // (a NaN's bits are above +inf's; the two halves of the wave hold all of a block's 32 tokens between them)
        bad = __any(sbits > 0x7f800000u);
        return total;
    }
};

template <class Form, bool MASKED, bool LISTED>
__global__ __launch_bounds__(NT) void token_index_scan_kernel(TokenScanArgs a) {
    static_assert(!(MASKED && LISTED), "a rescore tests live per id");
    static_assert(!LISTED || Form::LISTABLE, "the f16 form's rescore is token_index_pairs_kernel + maxsim_kernel");
    extern __shared__ __attribute__((aligned(16))) unsigned char ti_lds[];
    const int item = xcd_item();                 // (kernels.h: the queries of one slice go to one XCD and find its rows in that L2)
    if (item >= a.n_items) return;
    const int slice = item / a.nq, qi = item - slice * a.nq;
    const int k = a.k, L = a.L;
    // Code placement (DESIGN §16.3 "Measured"; §8.1: the shared selection kept both offsets).  With the same instructions in the same order the scan's time moves by 0.2 .. 1.3 % with the
    // byte offset of the round loop's code inside the kernel.  The plain instantiations therefore start with Form::PLAIN_PAD s_nop, once per
    // workgroup: their loops lie at the offsets they were measured at.  The numbers belong to this compiler's output for this source: a change
    // in front of the round loop drops them or derives them again from a measurement, it does not inherit them
    if constexpr (!MASKED && !LISTED) asm volatile(".rept %0\n\ts_nop 0\n\t.endr" ::"n"(Form::PLAIN_PAD));
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    Form f;
    float *ls = (float *)f.init(a, ti_lds);                    // behind the staged query: the list and the count
    int *li = (int *)(ls + L);
    const SelectLists sel{ls, li, li + L, L, k, L - k - TOKEN_STEP_DOCS};    // a step pushes at most TOKEN_STEP_DOCS entries
    // (everything up to the loop is uniform over the workgroup)
    const int q0 = a.qcu[qi], nq = a.qcu[qi + 1] - q0;
    const int n_list = LISTED ? a.n_cand : a.n_docs;           // what the slices cut: candidate positions, or documents
    const int r0 = (int)min((long long)slice * a.slice_docs, (long long)n_list);
    const int r1 = (int)min((long long)r0 + a.slice_docs, (long long)n_list);
    const size_t out = ((size_t)qi * a.n_slices + slice) * k;
    if (nq <= 0 || q0 < 0 || nq > a.max_q_len || r0 >= r1) {
        select_store_empty(a.ws_s, a.ws_i, out, k, tid);
        return;
    }
    const int nblk = (nq + TOKEN_QB - 1) / TOKEN_QB;
    [[maybe_unused]] const bool qbad = f.stage(a, qi, q0, nq, nblk, tid);
    select_init(sel, 1, tid);
    float ts = -INFINITY;
    int ti = SENT_ID;
    // (the staging's barrier; a query its form calls bad: the guards' lists)
    if constexpr (Form::BAD_QUERIES) {
        if (__syncthreads_or(qbad)) {
            select_store_empty(a.ws_s, a.ws_i, out, k, tid);
            return;
        }
    } else {
        __syncthreads();
    }

    for (int base = r0; base < r1; base += TOKEN_STEP_DOCS) {
        // MASKED: bit i of m = document base + i qualifies.  The step's documents lie in up to three mask words (a slice starts
        // anywhere); only words that hold a document below r1 are read, so none at or beyond ceil(n_docs / 32).  Everything here is
        // computed from the workgroup's values alone, the same in all four waves.
        [[maybe_unused]] uint64_t m = 0;
        if constexpr (MASKED) {
            const int wi = base >> 5, sh = base & 31, we = (min(base + TOKEN_STEP_DOCS, r1) - 1) >> 5;
            const uint32_t w0 = token_mask_word(a, wi);
            const uint32_t w1 = wi + 1 <= we ? token_mask_word(a, wi + 1) : 0u;
            const uint32_t w2 = wi + 2 <= we ? token_mask_word(a, wi + 2) : 0u;
            m = ((uint64_t)w1 << 32 | w0) >> sh;
            if (sh) m |= (uint64_t)w2 << (64 - sh);
            // a step without a qualifying document pushes nothing: the count is what the last look left, so select_step_end — both
            // barriers and the look — can go, for the whole workgroup, since m is the workgroup's
            if (m == 0) continue;
        }
        for (int u = 0; u < TOKEN_ROUNDS; ++u) {
            const int pos = base + NWAVE * u + wave;           // (wave-uniform)
            if (pos >= r1) break;
            int d = pos;
            if constexpr (MASKED) {
                // a document that does not qualify is skipped here, in front of its lengths and rows, inside the round loop: the wave
                // goes on to its next round and meets the step's barriers like the others, even when it scored nothing at all
                if (!(m >> (NWAVE * u + wave) & 1)) continue;
            }
            if constexpr (LISTED) {
                // (skipped inside the round loop, like a masked document)
                d = __builtin_amdgcn_readfirstlane(a.cand[(size_t)qi * a.n_cand + pos]);
                if (d < 0 || d >= a.n_docs) continue;
                if (a.live && !(__builtin_amdgcn_readfirstlane(a.live[d >> 5]) >> (d & 31) & 1u)) continue;
            }
            const int d0 = __builtin_amdgcn_readfirstlane(a.cu[d]), nd = __builtin_amdgcn_readfirstlane(a.cu[d + 1]) - d0;
            bool dbad;
            const float total = f.score(a, d0, nd, nq, nblk, lane, dbad);
            if (lane == 0 && !dbad && better(total, d, ts, ti)) select_push(sel, 0, total, d);
        }
        if (select_step_end(sel, 1, tid)) {
            select_threshold(sel, 0, ts, ti);
            select_resume(sel, 1, tid);
        }
    }
    select_finish(sel, 1, tid);
    for (int j = tid; j < k; j += NT) { a.ws_s[out + j] = ls[j]; a.ws_i[out + j] = li[j]; }
}

// One wave per row (device.h quantize_row_i8); the row addressing is TokenI8QuantizeArgs' (token_index_kernels.h)
template <class T>
__global__ __launch_bounds__(256) void token_i8_quantize_kernel(TokenI8QuantizeArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.n) return;                                      // (the whole wave)
    long long row = w;
    if (a.qcu) {
        const int qi = (int)(w / a.max_q_len), t = (int)(w - (long long)qi * a.max_q_len);
        const int q0 = a.qcu[qi], len = a.qcu[qi + 1] - q0;
        if (len <= 0 || q0 < 0 || len > a.max_q_len || t >= len) return;
        row = (long long)q0 + t;
    }
    quantize_row_i8((const T *)a.src + row * a.dim, a.dim, a.dpad, a.codes + w * a.dpad, a.scales + w, lane);
}

__global__ __launch_bounds__(256) void token_index_pairs_kernel(TokenPairsArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.nq * a.n_cand) return;
    const int id = a.cand[i];
    bool ok = id >= 0 && id < a.n_docs;
    if (ok && a.live) ok = (a.live[id >> 5] >> (id & 31)) & 1u;         // (a removed document: no candidate, as an id out of range)
    a.pairs[2 * i] = (int32_t)(i / a.n_cand);
    a.pairs[2 * i + 1] = ok ? id : -1;
    a.ws_i[i] = ok ? id : SENT_ID;
}

// Compaction (TokenGatherArgs): one wave per kept document, the documents dealt round over the launch's waves.  A document's rows
// are contiguous in both arrays, so a wave copies ONE run of len * dim / 8 16-byte pieces, a lane a piece, four pieces in flight per
// lane; the offsets are the wave's (scalar loads).  Both arrays are 16-byte aligned and dim is a multiple of 8.
constexpr int GATHER_NT = 256, GATHER_MAX_BLOCKS = 16384;

__global__ __launch_bounds__(GATHER_NT) void token_index_gather_kernel(TokenGatherArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = (int)gridDim.x * (GATHER_NT / 64), chunks = a.dim >> 3;
    for (int j = (int)blockIdx.x * (GATHER_NT / 64) + wave; j < a.n; j += waves) {
        const int t0 = a.dst_cu[j], len = a.dst_cu[j + 1] - t0;
        const u32x4 *src = (const u32x4 *)a.src + (size_t)a.src_cu[a.old_ids[j]] * chunks;
        u32x4 *dst = (u32x4 *)a.dst + (size_t)t0 * chunks;
        const long long n = (long long)len * chunks;
        long long p = lane;
        for (; p + 192 < n; p += 256) {
            const u32x4 v0 = src[p], v1 = src[p + 64], v2 = src[p + 128], v3 = src[p + 192];
            dst[p] = v0; dst[p + 64] = v1; dst[p + 128] = v2; dst[p + 192] = v3;
        }
        for (; p < n; p += 64) dst[p] = src[p];
    }
}

DeviceFlags g_token_scan_lds;

// rows per launch of the quantisation: 2^22 waves of 64 threads, far below the 2^32 a launch's thread count wraps at
constexpr long long QUANT_MAX_ROWS = 1ll << 22;

}  // namespace

void token_index_kernels_init() {
    // (beyond the 64 KiB a launch gets unasked; a launch that still cannot have it fails, and the search reports the launch error)
    configure_once(g_token_scan_lds, [] {
        bool ok = true;
        for (const void *f : {(const void *)token_index_scan_kernel<F16Form, false, false>, (const void *)token_index_scan_kernel<F16Form, true, false>,
                              (const void *)token_index_scan_kernel<I8Form, false, false>, (const void *)token_index_scan_kernel<I8Form, true, false>,
                              (const void *)token_index_scan_kernel<I8Form, false, true>})
            ok = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOKEN_LDS_MAX) == hipSuccess && ok;
        if (!ok) (void)hipGetLastError();                      // (not left behind for an unrelated call's check)
    });
}

void launch_token_scan(int dtype, const TokenScanArgs &a, hipStream_t s) {
    if (a.n_items <= 0) return;
    const int grid = xcd_grid(a.n_items);
    const size_t lds = token_scan_lds_bytes(a.dim, dtype, a.max_q_len, a.k);
    const bool masked = a.live || a.allow;
    if (dtype == 2) {
        if (a.cand) BERT_LAUNCH((token_index_scan_kernel<I8Form, false, true>), dim3(grid), dim3(NT), lds, s, a);
        else if (masked) BERT_LAUNCH((token_index_scan_kernel<I8Form, true, false>), dim3(grid), dim3(NT), lds, s, a);
        else BERT_LAUNCH((token_index_scan_kernel<I8Form, false, false>), dim3(grid), dim3(NT), lds, s, a);
    } else {
        // (cand is the int8 form's: TokenIndex scores an f16 rescore with maxsim)
        if (masked) BERT_LAUNCH((token_index_scan_kernel<F16Form, true, false>), dim3(grid), dim3(NT), lds, s, a);
        else BERT_LAUNCH((token_index_scan_kernel<F16Form, false, false>), dim3(grid), dim3(NT), lds, s, a);
    }
}

void launch_token_i8_quantize(const TokenI8QuantizeArgs &a, bool src_f32, hipStream_t s) {
    // (the queries' form is one launch: at most TokenIndex::QCHUNK * TOKEN_MAX_QUERY slots)
    for (long long r0 = 0; r0 < a.n; r0 += QUANT_MAX_ROWS) {
        TokenI8QuantizeArgs p = a;
        p.n = std::min(QUANT_MAX_ROWS, a.n - r0);
        if (!a.qcu) {
            p.src = (const char *)a.src + (size_t)r0 * a.dim * (src_f32 ? 4 : 2);
            p.codes = a.codes + (size_t)r0 * a.dpad;
            p.scales = a.scales + r0;
        }
        const dim3 grid((unsigned)((p.n + 3) / 4));
        if (src_f32) BERT_LAUNCH(token_i8_quantize_kernel<float>, grid, dim3(256), 0, s, p);
        else BERT_LAUNCH(token_i8_quantize_kernel<half_t>, grid, dim3(256), 0, s, p);
        if (a.qcu) break;
    }
}

void launch_token_gather(const TokenGatherArgs &a, hipStream_t s) {
    // (a wave per document, at most GATHER_MAX_BLOCKS blocks of four waves — 2^22 threads, far below the 2^32 a launch's thread count
    // wraps at —; the kernel's loop deals the documents beyond that over the same waves)
    if (a.n <= 0) return;
    const int blocks = std::min((a.n + GATHER_NT / 64 - 1) / (GATHER_NT / 64), GATHER_MAX_BLOCKS);
    BERT_LAUNCH(token_index_gather_kernel, dim3(blocks), dim3(GATHER_NT), 0, s, a);
}

void launch_token_pairs(const TokenPairsArgs &a, hipStream_t s) {
    // (nq <= TokenIndex::QCHUNK = 256 and n_cand <= TOKEN_MAX_CAND = 1024: at most 2^18 threads)
    const size_t n = (size_t)a.nq * a.n_cand;
    if (!n) return;
    BERT_LAUNCH(token_index_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace bert_hip
