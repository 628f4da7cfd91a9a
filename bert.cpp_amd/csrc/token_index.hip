// token_index.hip — the device code of the token index (gfx950; bert_hip.h "TOKEN INDEX"): documents' f16 token rows in HBM and their
// exact MaxSim top-k search.  The kernels and their launchers (token_index_kernels.h, which states the stored form); the TokenIndex
// class that plans and orders them is token_index.cpp (token_index.h).
//
//   token_index_scan_kernel  one workgroup of four waves per (query, slice of consecutive documents).  The workgroup stages ALL the
//                   query's blocks of 32 tokens in LDS once (rows of dim + 8 halfs, maxsim's padding: the 32 rows a ds_read_b128 step
//                   touches lie on distinct bank groups; the slots behind the query's end are zero-filled).  Then each wave takes whole
//                   documents of the slice — first + wave, first + wave + 4, ... —: per query block it walks the document's 32-token
//                   blocks straight from global memory / L2, runs score_chain_f16 with the document block as the A operand and the
//                   query block as the B operand, keeps the running elementwise max in 16 registers, masks only the document's last
//                   block, folds the 16 maxima, meets lane ^ 32 (xor32_max) and adds the block's 32 maxima with wave_sum_f32 — the
//                   expressions of maxsim_kernel, whose four waves' maxima meet by an exact max where here one wave saw them all.  No
//                   LDS exchange between waves: a document belongs to one wave, a short one costs one chain and one reduction.
//   Selection.      index_probe_kernel's for one query: a list of L (score, id) entries in LDS, the threshold in registers; lane 0
//                   of a wave pushes a document that beats the threshold; every TOKEN_ROUNDS documents per wave the workgroup looks
//                   at the count and sorts (bitonic_sort_lists) when the room left cannot hold another step's pushes.  The trip
//                   counts are the workgroup's — a wave without a document in a round scores nothing —, so every barrier is met by all
//                   four waves.  k entries per (query, slice) reach the workspace, which topk_merge_kernel merges; the scores never
//                   reach HBM.
//   Masking.        maxsim's: a document slot at or behind the document's end enters the max as -inf (its operand is zero-filled in
//                   registers, never read); a query slot at or behind the query's end adds +0.  No lane reads a row outside
//                   [cu[d], cu[d + 1]) of its document or outside the query's range.
//   Guards.         A query that is empty, descends, starts below 0 or is longer than the launch's max_q_len gets k entries of
//                   (-inf, INT_MAX) in every slice — id -1 / -INFINITY after the merge —; nothing else is touched.
//   Removed documents and allow-lists.  token_index_scan_kernel<true>: the same body with a 64-bit mask per step of TOKEN_STEP_DOCS
//                   documents, built from up to three words of live & allow that every wave loads through the scalar path.  A wave
//                   skips a document whose bit is clear before it reads the document's lengths or rows, INSIDE the round loop, so the
//                   step's barriers are met by all four waves whatever each of them scored; a step whose mask is zero is skipped by
//                   the whole workgroup, barriers included (the mask is the workgroup's, and nothing was pushed).  A step still
//                   pushes at most TOKEN_STEP_DOCS entries: L and the room rule are those of the unmasked kernel, whose instantiation
//                   <false> contains none of this.
//   token_index_pairs_kernel  a rescore's candidate ids as maxsim's pair list (token_index_kernels.h); a removed id is no candidate.
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

constexpr int SENT_ID = INT_MAX;        // id of an empty list entry (score -inf): ranks below every document, as in search.hip

static_assert(TOKEN_STEP_DOCS == 64, "the masked scan keeps a step's mask in one 64-bit word");

// the word of live & allow (a null pointer: all ones) at index wi, the same in every lane
__device__ __forceinline__ uint32_t token_mask_word(const TokenScanArgs &a, int wi) {
    uint32_t w = ~0u;
    if (a.live) w &= a.live[wi];
    if (a.allow) w &= a.allow[wi];
    return __builtin_amdgcn_readfirstlane(w);
}

template <bool MASKED>
__global__ __launch_bounds__(NT) void token_index_scan_kernel(TokenScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ti_lds[];
    // workgroup b runs on XCD b % 8: consecutive items — the queries of one slice — go to one XCD, so that they find the slice's rows
    // in that XCD's L2 (the grid is a multiple of 8; items beyond n_items do nothing)
    const int item = (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8);
    if (item >= a.n_items) return;
    const int slice = item / a.nq, qi = item - slice * a.nq;
    const int H = a.dim, ldq = H + 8, k = a.k, L = a.L;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, col = lane & 31, h = lane >> 5;
    half_t *qs = (half_t *)ti_lds;                                                         // [blocks of the launch][32][ldq]
    float *ls = (float *)(ti_lds + (size_t)((a.max_q_len + TOKEN_QB - 1) / TOKEN_QB) * TOKEN_QB * ldq * 2);
    int *li = (int *)(ls + L);
    int *cnt = li + L;
    // (everything up to the loop is uniform over the workgroup)
    const int q0 = a.qcu[qi], nq = a.qcu[qi + 1] - q0;
    const int r0 = (int)min((long long)slice * a.slice_docs, (long long)a.n_docs);
    const int r1 = (int)min((long long)r0 + a.slice_docs, (long long)a.n_docs);
    const size_t out = ((size_t)qi * a.n_slices + slice) * k;
    if (nq <= 0 || q0 < 0 || nq > a.max_q_len || r0 >= r1) {
        for (int j = tid; j < k; j += NT) { a.ws_s[out + j] = -INFINITY; a.ws_i[out + j] = SENT_ID; }
        return;
    }
    const int nblk = (nq + TOKEN_QB - 1) / TOKEN_QB, chunks = H >> 3;                      // (chunks: 16-byte pieces of a row)
    const f16x8 z = {};
    for (int i = tid; i < nblk * TOKEN_QB * chunks; i += NT) {
        const int r = i / chunks, c = i - r * chunks;
        *(f16x8 *)(qs + r * ldq + 8 * c) = r < nq ? *(const f16x8 *)(a.q + (size_t)(q0 + r) * H + 8 * c) : z;
    }
    for (int i = tid; i < L; i += NT) { ls[i] = -INFINITY; li[i] = SENT_ID; }
    if (tid == 0) *cnt = 0;
    float ts = -INFINITY;
    int ti = SENT_ID;
    __syncthreads();

    const int room = L - k - TOKEN_STEP_DOCS;                  // a step pushes at most TOKEN_STEP_DOCS entries
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
            // a step without a qualifying document pushes nothing: the count is what the last look left, so both barriers and the
            // look can go — for the whole workgroup, since m is the workgroup's
            if (m == 0) continue;
        }
        for (int u = 0; u < TOKEN_ROUNDS; ++u) {
            const int d = base + NWAVE * u + wave;             // (wave-uniform)
            if (d >= r1) break;
            if constexpr (MASKED) {
                // a document that does not qualify is skipped here, in front of its lengths and rows, inside the round loop: the wave
                // goes on to its next round and meets the step's barriers like the others, even when it scored nothing at all
                if (!(m >> (NWAVE * u + wave) & 1)) continue;
            }
            const int d0 = __builtin_amdgcn_readfirstlane(a.cu[d]), nd = __builtin_amdgcn_readfirstlane(a.cu[d + 1]) - d0;
            float total = 0.f;
            for (int qb = 0; qb < nblk; ++qb) {
                const bool qok = qb * TOKEN_QB + col < nq;
                const half_t *qrow = qs + (qb * TOKEN_QB + col) * ldq;
                f32x16 m;
#pragma unroll
                for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
                for (int j0 = 0; j0 < nd; j0 += 32) {
                    const bool dok = j0 + col < nd;            // this lane's row of the A operand: document token j0 + col
                    const half_t *drow = a.rows + (size_t)(d0 + (dok ? j0 + col : 0)) * H;
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
            if (lane == 0 && better(total, d, ts, ti)) {
                const int p = atomicAdd(cnt, 1);
                ls[k + p] = total;
                li[k + p] = d;
            }
        }
        __syncthreads();
        // (one thread reads the count between the two barriers: the next step's pushes come after the second)
        if (__syncthreads_or(tid == 0 && *cnt > room)) {
            bitonic_sort_lists(ls, li, 1, L, tid);
            ts = ls[k - 1];
            ti = li[k - 1];
            if (tid == 0) *cnt = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    if (__syncthreads_or(tid == 0 && *cnt > 0)) bitonic_sort_lists(ls, li, 1, L, tid);
    for (int j = tid; j < k; j += NT) { a.ws_s[out + j] = ls[j]; a.ws_i[out + j] = li[j]; }
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

}  // namespace

void token_index_kernels_init() {
    // (beyond the 64 KiB a launch gets unasked; a launch that still cannot have it fails, and the search reports the launch error)
    configure_once(g_token_scan_lds, [] {
        bool ok = true;
        for (const void *f : {(const void *)token_index_scan_kernel<false>, (const void *)token_index_scan_kernel<true>})
            ok = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOKEN_LDS_MAX) == hipSuccess && ok;
        if (!ok) (void)hipGetLastError();                      // (not left behind for an unrelated call's check)
    });
}

void launch_token_scan(const TokenScanArgs &a, hipStream_t s) {
    if (a.n_items <= 0) return;
    const int grid = (a.n_items + 7) / 8 * 8;                  // (the kernel's XCD map)
    const size_t lds = token_scan_lds_bytes(a.dim, a.max_q_len, a.k);
    if (a.live || a.allow) BERT_LAUNCH(token_index_scan_kernel<true>, dim3(grid), dim3(NT), lds, s, a);
    else BERT_LAUNCH(token_index_scan_kernel<false>, dim3(grid), dim3(NT), lds, s, a);
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
