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
//   token_index_pairs_kernel  a rescore's candidate ids as maxsim's pair list (token_index_kernels.h).
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
        for (int u = 0; u < TOKEN_ROUNDS; ++u) {
            const int d = base + NWAVE * u + wave;             // (wave-uniform)
            if (d >= r1) break;
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
    const bool ok = id >= 0 && id < a.n_docs;
    a.pairs[2 * i] = (int32_t)(i / a.n_cand);
    a.pairs[2 * i + 1] = ok ? id : -1;
    a.ws_i[i] = ok ? id : SENT_ID;
}

DeviceFlags g_token_scan_lds;

}  // namespace

void token_index_kernels_init() {
    // (beyond the 64 KiB a launch gets unasked; a launch that still cannot have it fails, and the search reports the launch error)
    configure_once(g_token_scan_lds, [] {
        if (hipFuncSetAttribute((const void *)token_index_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOKEN_LDS_MAX) != hipSuccess)
            (void)hipGetLastError();                           // (not left behind for an unrelated call's check)
    });
}

void launch_token_scan(const TokenScanArgs &a, hipStream_t s) {
    if (a.n_items <= 0) return;
    const int grid = (a.n_items + 7) / 8 * 8;                  // (the kernel's XCD map)
    BERT_LAUNCH(token_index_scan_kernel, dim3(grid), dim3(NT), token_scan_lds_bytes(a.dim, a.max_q_len, a.k), s, a);
}

void launch_token_pairs(const TokenPairsArgs &a, hipStream_t s) {
    // (nq <= TokenIndex::QCHUNK = 256 and n_cand <= TOKEN_MAX_CAND = 1024: at most 2^18 threads)
    const size_t n = (size_t)a.nq * a.n_cand;
    if (!n) return;
    BERT_LAUNCH(token_index_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace bert_hip
