// token_index_grouped.hip — the grouped scan of the f16 token index (gfx950; token_index_kernels.h TokenGroupScanArgs): one workgroup
// of four waves per (group of G <= 4 consecutive queries, slice of consecutive documents).  The ungrouped kernel (token_index.hip) reads
// every document row once per QUERY; this one reads it once per GROUP and scores it against all the group's staged query blocks.
//
//   Work map.       item = slice * n_groups + group through xcd_item(): the groups of one slice go to one XCD and find its rows in that L2.
//   LDS.            G * nbs block slots of 32 rows of dim + 8 halfs (nbs = ceil(max_q_len / 32): the launch knows no lengths; slot
//                   g * nbs + b is block b of query g; F16Form's padding), then the G lists' scores, their ids and the G counts.
//   Staging.        All the group's queries once; a query's blocks behind its last are neither staged nor used, the rows behind its end
//                   are zero-filled.  A query that fails the guards (empty, descending, start < 0, longer than max_q_len) stages
//                   nothing, scores nothing and is never pushed: its list stays select_init's (-inf, INT_MAX) and is stored as that.
//                   A group without a good query stores the empty lists and returns, as does an empty slice.
//   Scoring.        A document belongs to one wave — first + wave, + 4, ... — and no wave reads another's LDS.  The wave walks the slots
//                   in passes of NB = 4 (one pass where G * nbs <= 4); per pass the outer loop walks the document's 32-token blocks and the
//                   inner one k: score_chain_f16_shared_a with the document block as the A operand, requested from global memory / L2
//                   U = 8 steps ahead — the request crosses the block's end into the document's next block and the document's end into the
//                   first block of the wave's next document of the step, whose lengths were read through the scalar path in front of this
//                   document's chain — and one v_mfma_f32_32x32x16_f16 per step and live slot with the B operand read from LDS as it is
//                   used.  m[b] = fmaxf(m[b], acc[b]) per document block, the document's last block masked to -inf by F16Form's index
//                   expression; behind the last block, per slot in ascending order: the 16 maxima folded, xor32_max, and
//                   total[g] += wave_sum_f32(h == 0 && qok ? v : 0).  Every accumulator sees score_chain_f16's sequence and every total
//                   F16Form::score's sums in its order: a (query, document) score has the ungrouped kernel's bits, which are
//                   bert_hip_maxsim_device's.
//   Selection.      topk_select.h with nl = the group's queries, one threshold per query in registers; lane 0 pushes (total[g], d) into
//                   list g where it beats threshold g; a step pushes at most TOKEN_STEP_DOCS entries per list: L and the room rule are
//                   the ungrouped kernel's.  select_store writes the workspace [nq][n_slices][k] as the ungrouped kernel does.
//   MASKED.         The ungrouped kernel's step mask (token_scan_mask.h): skipped inside the round loop, a zero-mask step skipped by the
//                   whole workgroup.  A request ahead is only made for a document whose bit is set.
//   Bounds.         No lane reads a row outside [cu[d], cu[d + 1]) of a document of its slice or outside a good query's range.
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

constexpr int GROUP_NB = 4;                  // accumulators of a pass: the compile-time bound of the register arrays
constexpr int GROUP_U = 8;                   // steps of A fragments requested ahead

// (two workgroups a CU asked for: 64 accumulator registers, 64 running maxima and 2 x 4 U fragment registers come to 255 without a
// spill; left alone the compiler holds a whole group's LDS reads at once, takes 347 and one wave per SIMD)
template <bool MASKED>
__global__ __launch_bounds__(NT, 2) void token_index_scan_grouped_kernel(TokenGroupScanArgs a) {
    constexpr int G = TOKEN_MAX_GROUP, NB = GROUP_NB, U = GROUP_U;
    extern __shared__ __attribute__((aligned(16))) unsigned char tg_lds[];
    const int item = xcd_item();
    if (item >= a.n_items) return;
    // (everything up to the round loop is uniform over the workgroup)
    const int slice = item / a.n_groups, grp = item - slice * a.n_groups;
    const int qf = grp * a.group, gq = min(a.group, a.nq - qf);            // the group's first query and its queries
    const int k = a.k, L = a.L, H = a.dim, ldq = H + 8;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int col = lane & 31, h = lane >> 5;
    const int nbs = (a.max_q_len + TOKEN_QB - 1) / TOKEN_QB;
    half_t *qs = (half_t *)tg_lds;                                         // [a.group * nbs][32][ldq]
    float *ls = (float *)(tg_lds + (size_t)a.group * nbs * TOKEN_QB * ldq * 2);
    int *li = (int *)(ls + a.group * L);
    const SelectLists sel{ls, li, li + a.group * L, L, k, L - k - TOKEN_STEP_DOCS};
    const int r0 = (int)min((long long)slice * a.slice_docs, (long long)a.n_docs);
    const int r1 = (int)min((long long)r0 + a.slice_docs, (long long)a.n_docs);
    // the guards, per query: qn[g] = its tokens, 0 for a query that fails them or lies behind the group's end
    int qn[G], qb0[G];
    bool any = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        qn[g] = 0; qb0[g] = 0;
        if (g < gq) {
            const int q0 = a.qcu[qf + g], n = a.qcu[qf + g + 1] - q0;
            if (n > 0 && q0 >= 0 && n <= a.max_q_len) { qn[g] = n; qb0[g] = q0; any = true; }
        }
    }
    if (!any || r0 >= r1) {
        for (int g = 0; g < gq; ++g) select_store_empty(a.ws_s, a.ws_i, ((size_t)(qf + g) * a.n_slices + slice) * k, k, tid);
        return;
    }
    {
        const int chunks = H >> 3;                                         // (chunks: 16-byte pieces of a row)
        const half_t *q = (const half_t *)a.q;
        const f16x8 z = {};
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int n = qn[g], nblk = (n + TOKEN_QB - 1) / TOKEN_QB;
            half_t *dst = qs + (size_t)g * nbs * TOKEN_QB * ldq;
            for (int i = tid; i < nblk * TOKEN_QB * chunks; i += NT) {
                const int r = i / chunks, c = i - r * chunks;
                *(f16x8 *)(dst + r * ldq + 8 * c) = r < n ? *(const f16x8 *)(q + (size_t)(qb0[g] + r) * H + 8 * c) : z;
            }
        }
    }
    select_init(sel, gq, tid);
    float ts[G];
    int ti[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { ts[g] = -INFINITY; ti[g] = SENT_ID; }
    __syncthreads();

    const half_t *rows = (const half_t *)a.rows;
    const int nslots = gq * nbs;
    const f16x8 z = {};
    // this lane's eight elements of step kk of row j0 + col of the document at row d0 (nd rows): zeros, unread, behind either end
    auto frag = [&](int d0, int nd, int j0, int kk) __attribute__((always_inline)) {
        return j0 + col < nd && kk + 8 * h < H ? *(const f16x8 *)(rows + (size_t)(d0 + j0 + col) * H + kk + 8 * h) : z;
    };

    for (int base = r0; base < r1; base += TOKEN_STEP_DOCS) {
        [[maybe_unused]] uint64_t m = 0;
        if constexpr (MASKED) {
            m = token_step_mask(a, base, r1);
            // (nothing was pushed and the mask is the workgroup's: the step's barriers can go, for all four waves)
            if (m == 0) continue;
        }
        // a[] holds the first U steps of this round's document (pre), requested while the round before was scored
        f16x8 av[U];
        bool pre = false;
        int pd0 = 0, pnd = 0;
        for (int u = 0; u < TOKEN_ROUNDS; ++u) {
            const int d = base + NWAVE * u + wave;                         // (wave-uniform)
            if (d >= r1) break;
            if constexpr (MASKED) {
                // (inside the round loop: the wave meets the step's barriers whatever it scored; pre is false here)
                if (!(m >> (NWAVE * u + wave) & 1)) continue;
            }
            int d0 = pd0, nd = pnd;
            if (!pre) {
                d0 = __builtin_amdgcn_readfirstlane(a.cu[d]); nd = __builtin_amdgcn_readfirstlane(a.cu[d + 1]) - d0;
#pragma unroll
                for (int uu = 0; uu < U; ++uu) av[uu] = frag(d0, nd, 0, 16 * uu);
            }
            // the wave's next document of this step, if it has one: its lengths now, its first steps behind this document's last
            bool nx = u + 1 < TOKEN_ROUNDS && d + NWAVE < r1;
            if constexpr (MASKED) nx = nx && (m >> (NWAVE * (u + 1) + wave) & 1);
            if (nx) { pd0 = __builtin_amdgcn_readfirstlane(a.cu[d + NWAVE]); pnd = __builtin_amdgcn_readfirstlane(a.cu[d + NWAVE + 1]) - pd0; }

            float total[G] = {0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < nslots; s0 += NB) {
                // the pass's slots: sg[b] the query of slot s0 + b, st[b] its tokens in that block (<= 0: the slot is not live)
                int sg[NB], st[NB];
                {
                    int g = s0 / nbs, blk = s0 - g * nbs;
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        int n = 0;
#pragma unroll
                        for (int gg = 0; gg < G; ++gg) n = g == gg ? qn[gg] : n;
                        sg[b] = g;
                        st[b] = s0 + b < nslots ? n - TOKEN_QB * blk : 0;
                        if (++blk == nbs) { blk = 0; ++g; }
                    }
                }
                const bool last_pass = s0 + NB >= nslots;
                f32x16 mx[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx[b][r] = -INFINITY;
                const half_t *qrow = qs + (size_t)(s0 * TOKEN_QB + col) * ldq + 8 * h;
                if (s0 > 0) {
                    // (a later pass walks the document again: its first steps once more)
#pragma unroll
                    for (int uu = 0; uu < U; ++uu) av[uu] = frag(d0, nd, 0, 16 * uu);
                }
                for (int j0 = 0; j0 < nd; j0 += 32) {
                    f32x16 acc[NB];
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[b] = f32x16{};
                    const bool more = j0 + 32 < nd, ahead = !more && last_pass && nx;
                    score_chain_f16_shared_a<NB, U>(
                        [&](int kk, bool) __attribute__((always_inline)) { return frag(d0, nd, j0, kk); },
                        [&](int kk) __attribute__((always_inline)) { return more ? frag(d0, nd, j0 + 32, kk) : ahead ? frag(pd0, pnd, 0, kk) : z; },
                        [&](int b, int kk) __attribute__((always_inline)) {
                            return kk + 8 * h < H ? *(const f16x8 *)(qrow + (size_t)b * TOKEN_QB * ldq + kk) : z;
                        },
                        [&](int b) __attribute__((always_inline)) { return st[b] > 0; }, H, av, acc);
                    if (more) {
#pragma unroll
                        for (int b = 0; b < NB; ++b)
                            if (st[b] > 0) {
#pragma unroll
                                for (int r = 0; r < 16; ++r) mx[b][r] = __builtin_fmaxf(mx[b][r], acc[b][r]);
                            }
                    } else {
#pragma unroll
                        for (int b = 0; b < NB; ++b)
                            if (st[b] > 0) {
#pragma unroll
                                for (int r = 0; r < 16; ++r) {
                                    const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                                    mx[b][r] = __builtin_fmaxf(mx[b][r], j < nd ? acc[b][r] : -INFINITY);
                                }
                            }
                    }
                }
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (st[b] > 0) {
                        float v = mx[b][0];
#pragma unroll
                        for (int r = 1; r < 16; ++r) v = __builtin_fmaxf(v, mx[b][r]);
                        v = xor32_max(v);
                        const float x = wave_sum_f32(h == 0 && col < st[b] ? v : 0.f);
#pragma unroll
                        for (int gg = 0; gg < G; ++gg)
                            if (sg[b] == gg) total[gg] += x;
                    }
            }
            pre = nx;
            if (lane == 0) {
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (qn[g] > 0 && better(total[g], d, ts[g], ti[g])) select_push(sel, g, total[g], d);
            }
        }
        if (select_step_end(sel, gq, tid)) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < gq) select_threshold(sel, g, ts[g], ti[g]);
            select_resume(sel, gq, tid);
        }
    }
    select_finish(sel, gq, tid);
    select_store(sel, gq, a.ws_s, a.ws_i, qf, a.n_slices, slice, tid);
}

}  // namespace

const TokenGroupScanKernel *token_scan_grouped_kernels() {
    static constexpr TokenGroupScanKernel KERNELS[2] = {token_index_scan_grouped_kernel<false>, token_index_scan_grouped_kernel<true>};
    return KERNELS;
}

}  // namespace bert_hip
