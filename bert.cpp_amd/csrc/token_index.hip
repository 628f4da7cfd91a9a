// token_index.hip — the device code of the token index (gfx950; bert_hip.h "TOKEN INDEX", "TOKEN INDEX, int8 form" and "TOKEN INDEX,
// MXFP4 form"): documents' token rows in HBM — f16 rows, int8 codes with one f32 scale per token, or MXFP4 rows with their scales inside —
// and their exact MaxSim top-k search.  The kernels and their launchers (token_index_kernels.h, which states the three stored forms
// and their table); the TokenIndex class that plans and orders them is token_index.cpp (token_index.h).  The second scan kernel, the
// grouped scan of the f16 form, is token_index_grouped.hip; its two instantiations are launched and opted into the LDS from here
// (TOKEN_SCANS, launch_token_scan: the ten scan instantiations stated once).
//
//   token_index_scan_kernel<Form, MASKED, LISTED>  ONE skeleton — the work map, the guards, the list, the step mask, the round loop and
//                   its barriers, the selection, the write-out — stated once; a Form (F16Form, I8Form, Mxfp4Form) holds only how a query
//                   is staged in LDS and how one document is scored.  Eight instantiations: f16 plain and masked; int8 and mxfp4 plain,
//                   masked and listed.
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
//   LISTED.         A rescore (int8 and mxfp4 forms; the f16 form's is maxsim_kernel behind token_index_pairs_kernel): a slice is a range of
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
//   Mxfp4Form.      v_mfma_scale_f32_32x32x64_f8f6f4: dpad / 64 instructions per (query block, document block), every scale inside the chain.
//     Query.        MXFP8 rows (dpad e4m3 codes, dpad / 32 E8M0 scale bytes, zero to a multiple of 16) staged once, codes and scale bytes
//                   in one LDS row of token_mx_ldq bytes: an ODD number of 16-byte slots (one slot added where the row's count is even), so
//                   the 32 rows a ds_read_b128 step touches lie on distinct slots of the bank row — the int8 form's argument.
//     Score.        The document block is the A operand as e2m1 (cbsz 4, four registers): lane (col, h) feeds step s the 16 row bytes
//                   at 32 s + 16 h of token j0 + col — the 32 codes of block 2 s + h — straight from global memory / L2.  The query block
//                   is the B operand as e4m3 (blgp 0, eight registers): the 16 bytes at 64 s + 16 h and at 64 s + 32 + 16 h of query token
//                   col.  ScoreBlock<mxfp4_t>::run (search.hip) states the map with the roles the other way round; the scales go by
//                   k-block for either operand, so a lane reads each scale dword once, shifts it by 8 h, and opsel 0 / 2 serve every lane
//                   (the query's dwords once per query block, outside the document's loop).  tests/test_gpu_late_mxfp4.py's exact-fit
//                   test holds this map on the hardware.  U = 4 steps of loads in flight behind wave-uniform tests of dpad, the chain
//                   unrolled to the 16 steps of dim 1024.  acc[r] is document token j0 + (r & 3) + 8 (r >> 2) + 4 h against query token
//                   col — the f16 form's layout —, so the block's epilogue is the f16 form's 16 maxima and nothing else, and the max,
//                   the last block's -inf, xor32_max and wave_sum_f32 are its lines.
//     Non-finite.   The quantiser writes 0xFF into every scale byte of such a token and nothing else writes that byte.  stage looks at
//                   the first scale byte of every query token (a query with one: the guards' lists); score at the first scale byte of
//                   every document token, from the dwords it holds (such a document is never pushed) — not at what the MFMA makes of it.
//   token_mx_quantize_kernel  f32 or f16 rows -> MXFP4 rows (adds) or MXFP8 rows (queries), one wave per row by device.h's quantize_row_mx —
//                   the embedding index's rule, stated there once.
//   token_i8_quantize_kernel  f32 or f16 rows (f16 is converted exactly) -> codes and scales, one wave per row by device.h's
//                   quantize_row_i8 — the embedding index's rule, stated there once.
//                   Both take TokenQuantizeArgs and share token_quantize_src_row, the slot addressing and the guards: they serve the
//                   adds and, with qcu, the queries of every search and rescore, through one launcher (launch_token_quantize).
//   token_index_pairs_kernel  an f16 rescore's candidate ids as maxsim's pair list (token_index_kernels.h); a removed id is no candidate.
//   token_index_gather_kernel  compaction: the kept documents' rows into a fresh allocation (see the kernel).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "device.h"
#include "score_chain.h"
#include "token_index_kernels.h"
#include "token_scan_mask.h"
#include "topk_select.h"

namespace bert_hip {

namespace {

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

// v_mfma_scale_f32_32x32x64_f8f6f4 with the roles of ScoreBlock<mxfp4_t>::run (search.hip) the other way round, so that the maximum over
// a document's tokens stays in registers: A = the document block's e2m1 codes (cbsz 4), B = the staged query block's e4m3 codes (blgp 0).
struct Mxfp4Form {
    static constexpr bool LISTABLE = true;
    static constexpr bool BAD_QUERIES = true;           // (a query with a non-finite token: 0xFF scale bytes)
    static constexpr int PLAIN_PAD = 0;                 // (no placement was measured for this form)
    static constexpr int U = 4, MAX_SC = MAXSIM_MAX_H / 128;      // steps of loads in flight; scale dwords of a row (16 steps)
    uint8_t *qs;                                        // [blocks of the launch][32][ldq]
    int P, ldq, qbytes, rb;                             // qbytes: a query's MXFP8 row in the workspace; rb: a stored row

    __device__ __forceinline__ unsigned char *init(const TokenScanArgs &a, unsigned char *lds) {
        P = a.dpad; ldq = token_mx_ldq(a.dim); qbytes = (int)token_mx_query_bytes(a.dim); rb = (int)token_mx_row_bytes(a.dim);
        qs = lds;
        return lds + (size_t)((a.max_q_len + TOKEN_QB - 1) / TOKEN_QB) * TOKEN_QB * ldq;
    }
    __device__ __forceinline__ bool stage(const TokenScanArgs &a, int qi, int, int nq, int nblk, int tid) const {
        const int chunks = qbytes >> 4, sc = P >> 4;    // (chunks: 16-byte pieces of a row; piece sc starts with the first scale byte)
        const i32x4 z = {};
        const uint8_t *qsrc = (const uint8_t *)a.q + (size_t)qi * a.max_q_len * qbytes;
        bool qbad = false;
        for (int i = tid; i < nblk * TOKEN_QB * chunks; i += NT) {
            const int r = i / chunks, c = i - r * chunks;
            const i32x4 v = r < nq ? *(const i32x4 *)(qsrc + (size_t)r * qbytes + 16 * c) : z;
            *(i32x4 *)(qs + r * ldq + 16 * c) = v;
            qbad |= c == sc && (v[0] & 0xff) == 0xff;
        }
        return qbad;
    }
    __device__ __forceinline__ float score(const TokenScanArgs &a, int d0, int nd, int nq, int nblk, int lane, bool &bad) const {
        const int col = lane & 31, h = lane >> 5;
        const uint8_t *rows = (const uint8_t *)a.rows;
        const i32x4 z = {};
        float total = 0.f;
        bool dbad = false;
        for (int qb = 0; qb < nblk; ++qb) {
            const bool qok = qb * TOKEN_QB + col < nq;
            // (a staged slot behind the query's end is zero-filled: codes 0 under the scale 2^-127, every product +0)
            const uint8_t *qrow = qs + (qb * TOKEN_QB + col) * ldq;
            // the query token's scale dwords, the same for every block of the document: dword j holds blocks 4 j .. 4 j + 3, steps
            // 2 j and 2 j + 1; shifted by 8 h, byte 0 is block 4 j + h (step 2 j, opsel 0) and byte 2 block 4 j + 2 + h (step 2 j + 1, opsel 2)
            uint32_t qsc[MAX_SC];
#pragma unroll
            for (int j = 0; j < MAX_SC; ++j) qsc[j] = 128 * j < P ? *(const uint32_t *)(qrow + P + 4 * j) >> (8 * h) : 0u;
            f32x16 m;
#pragma unroll
            for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
            for (int j0 = 0; j0 < nd; j0 += 32) {
                const bool dok = j0 + col < nd;            // this lane's row of the A operand: document token j0 + col
                const uint8_t *drow = rows + (size_t)(d0 + (dok ? j0 + col : 0)) * rb;
                uint32_t dsc[MAX_SC];
#pragma unroll
                for (int j = 0; j < MAX_SC; ++j) dsc[j] = dok && 128 * j < P ? *(const uint32_t *)(drow + (P >> 1) + 4 * j) : 0u;
                // (a finite row holds no 0xFF scale byte, a non-finite one nothing else; the columns of the blocks are all the tokens)
                dbad |= (dsc[0] & 0xffu) == 0xffu;
#pragma unroll
                for (int j = 0; j < MAX_SC; ++j) dsc[j] >>= 8 * h;
                f32x16 acc = {};
#pragma unroll
                for (int g = 0; g < MAX_SC / 2; ++g) {
                    if (256 * g >= P) break;               // (wave-uniform)
                    i32x4 av[U], bv[U][2];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const bool in = 256 * g + 64 * u < P;
                        const uint8_t *qk = qrow + 256 * g + 64 * u + 16 * h;
                        av[u] = dok && in ? *(const i32x4 *)(drow + 128 * g + 32 * u + 16 * h) : z;
                        bv[u][0] = in ? *(const i32x4 *)qk : z;
                        bv[u][1] = in ? *(const i32x4 *)(qk + 32) : z;
                    }
                    // (the opsel is an immediate of the instruction: a compile-time loop)
                    static_for<U>([&](auto uc) __attribute__((always_inline)) {
                        constexpr int u = decltype(uc)::value;
                        if (256 * g + 64 * u < P) {
                            const i32x8 a8 = {av[u][0], av[u][1], av[u][2], av[u][3], 0, 0, 0, 0};
                            const i32x8 b8 = {bv[u][0][0], bv[u][0][1], bv[u][0][2], bv[u][0][3], bv[u][1][0], bv[u][1][1], bv[u][1][2], bv[u][1][3]};
                            acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc, 4, 0, 2 * (u & 1), (int)dsc[2 * g + (u >> 1)],
                                                                                  2 * (u & 1), (int)qsc[2 * g + (u >> 1)]);
                        }
                    });
                }
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
        bad = __any(dbad);
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
    if constexpr (!MASKED && !LISTED && Form::PLAIN_PAD > 0) asm volatile(".rept %0\n\ts_nop 0\n\t.endr" ::"n"(Form::PLAIN_PAD));
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
        // MASKED: bit i of m = document base + i qualifies (token_scan_mask.h), the same in all four waves
        [[maybe_unused]] uint64_t m = 0;
        if constexpr (MASKED) {
            m = token_step_mask(a, base, r1);
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

// The slot addressing and the guards of both quantisers (TokenQuantizeArgs, token_index_kernels.h): the row of src that slot w
// takes, or -1: the slot is left alone
__device__ __forceinline__ long long token_quantize_src_row(long long w, const int32_t *qcu, int max_q_len) {
    if (!qcu) return w;
    const int qi = (int)(w / max_q_len), t = (int)(w - (long long)qi * max_q_len);
    const int q0 = qcu[qi], len = qcu[qi + 1] - q0;
    return len <= 0 || q0 < 0 || len > max_q_len || t >= len ? -1 : (long long)q0 + t;
}

// One wave per row (device.h quantize_row_i8)
template <class T>
__global__ __launch_bounds__(256) void token_i8_quantize_kernel(TokenQuantizeArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.n) return;                                      // (the whole wave)
    const long long row = token_quantize_src_row(w, a.qcu, a.max_q_len);
    if (row < 0) return;
    quantize_row_i8((const T *)a.src + row * a.dim, a.dim, a.dpad, (int8_t *)a.dst + w * a.dpad, a.scales + w, lane);
}

// One wave per row (device.h quantize_row_mx, two passes: dim <= MAXSIM_MAX_H)
template <class T, bool FP8>
__global__ __launch_bounds__(256) void token_mx_quantize_kernel(TokenQuantizeArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.n) return;                                      // (the whole wave)
    const long long row = token_quantize_src_row(w, a.qcu, a.max_q_len);
    if (row < 0) return;
    quantize_row_mx<FP8, MAXSIM_MAX_H / 512>((const T *)a.src + row * a.dim, a.dim, a.dpad, (uint8_t *)a.dst + w * mx_row_bytes(FP8 ? a.dpad : a.dpad >> 1, a.dpad), lane);
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

// The instantiations of token_index_scan_kernel, stated once: [the form's row of TOKEN_FORMS][plain, masked, listed] (null: the f16
// form's rescore is maxsim's).  token_scan_grouped_kernels() (token_index_grouped.hip) holds the other two of the ten
using TokenScanKernel = void (*)(TokenScanArgs);
constexpr TokenScanKernel TOKEN_SCANS[3][3] = {
    {token_index_scan_kernel<F16Form, false, false>, token_index_scan_kernel<F16Form, true, false>, nullptr},
    {token_index_scan_kernel<I8Form, false, false>, token_index_scan_kernel<I8Form, true, false>, token_index_scan_kernel<I8Form, false, true>},
    {token_index_scan_kernel<Mxfp4Form, false, false>, token_index_scan_kernel<Mxfp4Form, true, false>, token_index_scan_kernel<Mxfp4Form, false, true>},
};

// rows per launch of the quantisation: 2^22 waves of 64 threads, far below the 2^32 a launch's thread count wraps at
constexpr long long QUANT_MAX_ROWS = 1ll << 22;

}  // namespace

void token_index_kernels_init() {
    // (beyond the 64 KiB a launch gets unasked; a launch that still cannot have it fails, and the search reports the launch error)
    configure_once(g_token_scan_lds, [] {
        bool ok = true;
        auto opt_in = [&](const void *f) { ok = (!f || hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOKEN_LDS_MAX) == hipSuccess) && ok; };
        for (const auto &form : TOKEN_SCANS)
            for (const TokenScanKernel f : form) opt_in((const void *)f);
        for (int m = 0; m < 2; ++m) opt_in((const void *)token_scan_grouped_kernels()[m]);
        if (!ok) (void)hipGetLastError();                      // (not left behind for an unrelated call's check)
    });
}

const char *token_scan_label(int dtype, const TokenGroupScanArgs &a) {
    const TokenForm &f = *token_form(dtype);
    const bool masked = a.live || a.allow;
    return a.group >= 2 ? f.grouped[masked] : a.cand ? f.rescore : f.scan[masked];
}

void launch_token_scan(int dtype, const TokenGroupScanArgs &a, hipStream_t s) {
    if (a.n_items <= 0) return;
    const int grid = xcd_grid(a.n_items);
    const bool masked = a.live || a.allow;
    if (a.group >= 2) {
        const TokenGroupScanKernel f = token_scan_grouped_kernels()[masked];
        BERT_LAUNCH(f, dim3(grid), dim3(NT), token_group_lds_bytes(a.dim, a.max_q_len, a.k, a.group), s, a);
        return;
    }
    // (a.cand: the LISTED instantiation, which the f16 form has none of: TokenIndex scores its rescore with maxsim)
    const TokenScanKernel f = TOKEN_SCANS[token_form(dtype) - TOKEN_FORMS][a.cand ? 2 : masked];
    BERT_LAUNCH(f, dim3(grid), dim3(NT), token_scan_lds_bytes(a.dim, dtype, a.max_q_len, a.k), s, (const TokenScanArgs &)a);
}

void launch_token_quantize(TokenQuant target, const TokenQuantizeArgs &a, bool src_f32, hipStream_t s) {
    using Kernel = void (*)(TokenQuantizeArgs);
    static constexpr Kernel KERNELS[3][2] = {{token_i8_quantize_kernel<half_t>, token_i8_quantize_kernel<float>},
                                             {token_mx_quantize_kernel<half_t, false>, token_mx_quantize_kernel<float, false>},
                                             {token_mx_quantize_kernel<half_t, true>, token_mx_quantize_kernel<float, true>}};
    const size_t rb = TOKEN_QUANT_ROW_BYTES[target](a.dim);
    // (the queries' form is one launch: at most TokenIndex::QCHUNK * TOKEN_MAX_QUERY slots)
    for (long long r0 = 0; r0 < a.n; r0 += QUANT_MAX_ROWS) {
        TokenQuantizeArgs p = a;
        p.n = std::min(QUANT_MAX_ROWS, a.n - r0);
        if (!a.qcu) {
            p.src = (const char *)a.src + (size_t)r0 * a.dim * (src_f32 ? 4 : 2);
            p.dst = (char *)a.dst + (size_t)r0 * rb;
            if (a.scales) p.scales = a.scales + r0;
        }
        const Kernel f = KERNELS[target][src_f32];
        BERT_LAUNCH(f, dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, s, p);
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
