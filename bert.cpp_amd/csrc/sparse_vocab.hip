// sparse_vocab.hip — learned sparse embeddings (gfx950; bert_hip.h "learned sparse embeddings"): from the MLM transform t [T][H] of a
// pass's packed token rows and the tied vocabulary matrix e [V][H] to one non-negative weight per sentence and vocabulary entry,
//   out[b][v] = z > 0 ? log1pf(z) : +0,   z = (max over the tokens i of sentence b of <t_i, e_v>) + bias[v],
// without the logits [T][V] ever leaving the chip.
//
//   sparse_vocab_kernel  the matrix-core form, H % 8 == 0, H <= 1024.  A workgroup of 4 waves owns one tile of consecutive packed token
//                        slots — 128 where 128 rows of H + 8 halfs fit the LDS (H <= 624), else 64 — and one slab of 32-entry
//                        vocabulary blocks.  The tile's rows are staged once in LDS (maxsim.hip's padding); a slot at or behind the
//                        served range is zero-filled, never read.  A wave takes the slab's blocks in pairs (2 w, 2 w + 1), (2 w + 8,
//                        2 w + 9), ...: the two blocks' rows go from L2 to registers once per k-step as B operands of
//                        score_chain_f16_grid (score_chain.h) and meet every 32-slot sub-block of the tile from LDS as A operand — 2 x 4
//                        accumulators at 128 slots, so a 16-byte LDS read feeds two matrix instructions and a 16-byte global read four.
//                        Lane (c, h) then holds vocabulary entry v0 + c against slots (r & 3) + 8 (r >> 2) + 4 h of sub-block s in
//                        register r of accumulator s.
//   Epilogue.            The max over a sentence's tokens is in-lane.  bnd[j] in LDS is the first slot of the tile's j-th sentence
//                        (bnd of the next one its end); the wave walks them in a uniform loop: a sub-block inside the sentence takes
//                        the plain 16-register fold, one with a boundary selects -inf per register, one outside is skipped; then
//                        xor32_max, + bias[v] (one f32 add), and lanes 0 .. 31 hold 32 consecutive vocabulary entries.
//   Combining.           A sentence may span tiles: a positive z goes to out by an integer atomic max on its bits (unsigned order is
//                        float order on non-negative floats; max is exact and commutative, so no bit depends on who arrives first);
//                        z <= 0 or NaN writes nothing, the launch's own zero-fill (hipMemsetAsync, capture-safe) stands for +0.
//                        fmaxf drops a NaN product.  sparse_finish_kernel applies log1pf in place.
//   Bits.                A sentence's row depends on its own token rows, the vocabulary rows and the bias alone: every product is its
//                        own chain, the max is exact.  Batch, place in the stream, grid, tile and slab do not enter.
//   sparse_vocab_f32_kernel  the plain form, any H: one workgroup per (sentence, 64 vocabulary entries); wave w takes 16 of them, a
//                        lane's fmaf chain over k = lane, lane + 64, ..., wave_sum_f32 per token, fmaxf over the tokens, the same
//                        bias / relu / log1pf, plain stores.  X / W: the rows and the matrix as f32 (the f32 route) or f16.
//   sparse_topk_kernel   one workgroup per dense row: the k largest positive weights, larger first, equal weights smaller id first.
//                        Keys (weight bits << 24 | 0xFFFFFF - id) are unique, so a radix select (7 passes of 8 bits, LDS histogram)
//                        finds the k-th largest key exactly, the keys at or above it are collected and sorted (bitonic, 256 slots).
#include <hip/hip_runtime.h>

#include <cmath>

#include "device.h"
#include "score_chain.h"

namespace bert_hip {

namespace {

constexpr int SV_WAVES = 4, SV_NT = 64 * SV_WAVES, SV_NB = 2;

// the sentences served, as a token range clamped to the rows that exist
__device__ __forceinline__ void served_range(const SparseVocabArgs &a, int &tbeg, int &tend) {
    tbeg = max(a.cu[a.s0], 0);
    tend = min(a.cu[a.s0 + a.ns], a.T);
}

template <int SUBS>
__global__ __launch_bounds__(SV_NT) void sparse_vocab_kernel(SparseVocabArgs a, int slab_blocks) {
    constexpr int TILE = 32 * SUBS;
    extern __shared__ __attribute__((aligned(16))) unsigned char sv_lds[];
    const int H = a.H, ld = H + 8;                             // (halfs per staged row)
    half_t *rs = (half_t *)sv_lds;                             // [TILE][ld]
    int *bnd = (int *)(sv_lds + (size_t)TILE * ld * 2);        // [TILE + 1]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, col = lane & 31, h = lane >> 5;
    const int s_end = a.s0 + a.ns;
    int tbeg, tend;
    served_range(a, tbeg, tend);
    const long long t0l = (long long)tbeg + (long long)blockIdx.x * TILE;
    if (t0l >= tend) return;                                   // (uniform: a tile behind the served tokens)
    const int t0 = (int)t0l, tile_n = min(TILE, tend - t0);
    int sf = a.s0, hi = s_end;                                 // the tile's first sentence: the largest s with cu[s] <= t0
    while (hi - sf > 1) {
        const int mid = (sf + hi) >> 1;
        if (a.cu[mid] <= t0) sf = mid; else hi = mid;
    }
    for (int j = tid; j <= TILE; j += SV_NT) bnd[j] = min(max(a.cu[min(sf + j, s_end)] - t0, 0), tile_n);
    const int chunks = H >> 3;                                 // 16-byte pieces of a row
    const f16x8 z8 = {};
    for (int i = tid; i < TILE * chunks; i += SV_NT) {
        const int r = i / chunks, c = i - r * chunks;
        *(f16x8 *)(rs + r * ld + 8 * c) = r < tile_n ? *(const f16x8 *)(a.t16 + (size_t)(t0 + r) * H + 8 * c) : z8;
    }
    __syncthreads();
    const half_t *arow = rs + col * ld + 8 * h;
    const int nblk = (a.V + 31) >> 5, blk0 = blockIdx.y * slab_blocks, blk_end = min(blk0 + slab_blocks, nblk);
    for (int blk = blk0 + wave * SV_NB; blk < blk_end; blk += SV_WAVES * SV_NB) {
        bool fok[SV_NB];                                       // this lane's row of B operand n: vocabulary entry 32 (blk + n) + col
        const half_t *erow[SV_NB];
#pragma unroll
        for (int n = 0; n < SV_NB; ++n) {
            fok[n] = blk + n < blk_end && 32 * (blk + n) + col < a.V;
            erow[n] = a.e16 + (size_t)(fok[n] ? 32 * (blk + n) + col : 0) * H + 8 * h;
        }
        f32x16 acc[SV_NB][SUBS] = {};
        score_chain_f16_grid<SUBS, SV_NB>(
            [&](int s, int k, bool) __attribute__((always_inline)) { return k + 8 * h < H ? *(const f16x8 *)(arow + s * 32 * ld + k) : z8; },
            [&](int n, int k, bool in) __attribute__((always_inline)) { return fok[n] && in && k + 8 * h < H ? *(const f16x8 *)(erow[n] + k) : z8; },
            H, acc);
#pragma unroll
        for (int n = 0; n < SV_NB; ++n) {
            if (blk + n >= blk_end) break;                     // (uniform)
            const int v = 32 * (blk + n) + col;
            const float bias = h == 0 && v < a.V ? a.bias[v] : 0.f;
            for (int j = 0; j < TILE && sf + j < s_end; ++j) {
                const int lo = __builtin_amdgcn_readfirstlane(bnd[j]), up = __builtin_amdgcn_readfirstlane(bnd[j + 1]);
                if (lo >= tile_n) break;
                if (up <= lo) continue;
                float m = -INFINITY;
#pragma unroll
                for (int s = 0; s < SUBS; ++s) {
                    if (up <= 32 * s || lo >= 32 * s + 32) continue;
                    if (lo <= 32 * s && up >= 32 * s + 32) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) m = __builtin_fmaxf(m, acc[n][s][r]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int slot = 32 * s + (r & 3) + 8 * (r >> 2) + 4 * h;
                            m = __builtin_fmaxf(m, slot >= lo && slot < up ? acc[n][s][r] : -INFINITY);
                        }
                    }
                }
                m = xor32_max(m);
                const float zv = m + bias;
                if (h == 0 && v < a.V && zv > 0.f) atomicMax((unsigned *)a.out + (size_t)(sf + j - a.s0) * a.V + v, __float_as_uint(zv));
            }
        }
    }
}

__global__ __launch_bounds__(256) void sparse_finish_kernel(float *out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = log1pf(out[i]);
}

constexpr int SF_VPB = 64;                                     // vocabulary entries per workgroup of the plain form

template <class X, class W>
__global__ __launch_bounds__(SV_NT) void sparse_vocab_f32_kernel(SparseVocabArgs a, const X *__restrict__ t, const W *__restrict__ e) {
    const int H = a.H, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int i0 = max(a.cu[a.s0 + b], 0), i1 = min(a.cu[a.s0 + b + 1], a.T);
    for (int v = blockIdx.x * SF_VPB + wave; v < min(a.V, (int)(blockIdx.x + 1) * SF_VPB); v += SV_WAVES) {
        const W *w = e + (size_t)v * H;
        float m = -INFINITY;
        for (int i = i0; i < i1; ++i) {
            const X *x = t + (size_t)i * H;
            float s = 0.f;
            for (int k = lane; k < H; k += 64) s = fmaf((float)x[k], (float)w[k], s);
            m = __builtin_fmaxf(m, wave_sum_f32(s));
        }
        const float zv = m + a.bias[v];
        if (lane == 0) a.out[(size_t)b * a.V + v] = zv > 0.f ? log1pf(zv) : 0.f;
    }
}

__global__ __launch_bounds__(256) void sparse_topk_kernel(const float *__restrict__ w, int V, int k, int32_t *__restrict__ ids, float *__restrict__ weights) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sel[256], s_prefix;
    __shared__ int s_rem, s_cnt;
    const float *row = w + (size_t)blockIdx.x * V;
    const int tid = threadIdx.x;
    auto key_of = [&](float x, int v) { return ((unsigned long long)__float_as_uint(x) << 24) | (unsigned long long)(0xFFFFFF - v); };
    // the k-th largest key, 8 bits a pass from the top of its 56: `prefix` the bits found so far, `rem` its rank among the keys that share them
    unsigned long long prefix = 0;
    int rem = k;
    for (int pass = 0; pass < 7; ++pass) {
        const int shift = 48 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (int v = tid; v < V; v += 256) {
            const float x = row[v];
            if (x > 0.f) {
                const unsigned long long key = key_of(x, v);
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned c = 0;
            int bin = 255;
            for (; bin >= 0; --bin) {
                if (c + hist[bin] >= (unsigned)rem) break;
                c += hist[bin];
            }
            s_rem = bin < 0 ? -1 : rem - (int)c;               // (-1, in the first pass only: fewer than k positive weights, all are taken)
            s_prefix = (prefix << 8) | (unsigned long long)(bin < 0 ? 0 : bin);
        }
        __syncthreads();
        rem = s_rem;
        prefix = rem < 0 ? 0 : s_prefix;
        if (rem < 0) break;                                    // (uniform)
    }
    sel[tid] = 0;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int v = tid; v < V; v += 256) {
        const float x = row[v];
        if (x > 0.f) {
            const unsigned long long key = key_of(x, v);
            if (key >= prefix) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < 256) sel[slot] = key;               // (at most k <= 256 keys reach here: they are unique)
            }
        }
    }
    // descending, whatever order the slots were drawn in
    for (int size = 2; size <= 256; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            const int partner = tid ^ stride;
            if (partner > tid) {
                const bool desc = (tid & size) == 0;
                const unsigned long long x = sel[tid], y = sel[partner];
                if ((x < y) == desc) { sel[tid] = y; sel[partner] = x; }
            }
        }
    __syncthreads();
    if (tid < k) {
        const unsigned long long key = sel[tid];
        ids[(size_t)blockIdx.x * k + tid] = key ? (int32_t)(0xFFFFFF - (unsigned)(key & 0xFFFFFF)) : -1;
        weights[(size_t)blockIdx.x * k + tid] = __uint_as_float((unsigned)(key >> 24));
    }
}

DeviceFlags g_sparse_configured[2];

int tile_slots(int H) { return H <= 624 ? 128 : 64; }         // 128 rows of H + 8 halfs and the boundaries within 160 KiB

bool common_ok(const SparseVocabArgs &a) { return a.ns > 0 && a.s0 >= 0 && a.T > 0 && a.H > 0 && a.V > 0 && a.bias && a.cu && a.out; }

}  // namespace

bool sparse_vocab_mfma_supported(int H) { return H >= 8 && H % 8 == 0 && H <= SPARSE_MFMA_MAX_H; }

size_t sparse_vocab_lds_bytes(int H) { return (size_t)tile_slots(H) * (H + 8) * 2 + (size_t)(tile_slots(H) + 1) * sizeof(int); }

// The launch geometry of the matrix-core form, host arithmetic alone: tokens per tile, token tiles, vocabulary blocks per slab, slabs.
bool sparse_vocab_geometry(int H, int V, int T, int ns, int max_len, SparseVocabGeometry &g) {
    g = SparseVocabGeometry{0, 0, 0, 0};
    if (ns <= 0 || T <= 0 || V <= 0 || max_len <= 0 || !sparse_vocab_mfma_supported(H)) return false;
    const int tile = tile_slots(H), nblk = (V + 31) / 32;
    const long long tokens = std::min<long long>(T, (long long)ns * max_len), n_tiles = (tokens + tile - 1) / tile;
    // slabs of whole wave rounds (8 blocks), sized so that a small batch still spreads over the chip: about a thousand workgroups or more
    const long long slabs_wanted = std::max<long long>(1, (1024 + n_tiles - 1) / n_tiles);
    const int slab_blocks = (int)std::min<long long>(64, std::max<long long>(8, ((nblk + slabs_wanted - 1) / slabs_wanted + 7) / 8 * 8));
    const int n_slabs = (nblk + slab_blocks - 1) / slab_blocks;
    if (n_slabs > GRID_YZ_MAX || n_tiles > 0x7FFFFFFF) return false;
    g = SparseVocabGeometry{tile, (int)n_tiles, slab_blocks, n_slabs};
    return true;
}

bool launch_sparse_vocab(const SparseVocabArgs &a, hipStream_t s) {
    SparseVocabGeometry g;
    if (!common_ok(a) || !a.t16 || !a.e16 || !sparse_vocab_geometry(a.H, a.V, a.T, a.ns, a.max_len, g)) return false;
    const int tile = g.tile, slab_blocks = g.slab_blocks;
    if (hipMemsetAsync(a.out, 0, (size_t)a.ns * a.V * sizeof(float), s) != hipSuccess) return false;
    const dim3 grid((unsigned)g.n_tiles, (unsigned)g.n_slabs);
    // (past the 64 KiB a kernel gets without asking from H = 248 on: 100 868 bytes at H = 384, 132 356 at H = 1024)
    if (tile == 128) {
        configure_once(g_sparse_configured[0], [] { (void)hipFuncSetAttribute((const void *)sparse_vocab_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sparse_vocab_lds_bytes(624)); });
        BERT_LAUNCH(sparse_vocab_kernel<4>, grid, dim3(SV_NT), sparse_vocab_lds_bytes(a.H), s, a, slab_blocks);
    } else {
        configure_once(g_sparse_configured[1], [] { (void)hipFuncSetAttribute((const void *)sparse_vocab_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sparse_vocab_lds_bytes(SPARSE_MFMA_MAX_H)); });
        BERT_LAUNCH(sparse_vocab_kernel<2>, grid, dim3(SV_NT), sparse_vocab_lds_bytes(a.H), s, a, slab_blocks);
    }
    return true;
}

void launch_sparse_finish(float *out, size_t n, hipStream_t s) {
    if (!n) return;
    BERT_LAUNCH(sparse_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, n);
}

bool launch_sparse_vocab_f32(const SparseVocabArgs &a, hipStream_t s) {
    if (!common_ok(a) || (!a.t32 && !a.t16) || (!a.e32 && !a.e16) || a.ns > GRID_YZ_MAX) return false;
    const dim3 grid((unsigned)((a.V + SF_VPB - 1) / SF_VPB), (unsigned)a.ns);
    if (a.t32 && a.e32) BERT_LAUNCH((sparse_vocab_f32_kernel<float, float>), grid, dim3(SV_NT), 0, s, a, a.t32, a.e32);
    else if (a.t32) BERT_LAUNCH((sparse_vocab_f32_kernel<float, half_t>), grid, dim3(SV_NT), 0, s, a, a.t32, a.e16);
    else if (a.e32) BERT_LAUNCH((sparse_vocab_f32_kernel<half_t, float>), grid, dim3(SV_NT), 0, s, a, a.t16, a.e32);
    else BERT_LAUNCH((sparse_vocab_f32_kernel<half_t, half_t>), grid, dim3(SV_NT), 0, s, a, a.t16, a.e16);
    return true;
}

bool launch_sparse_topk(const float *w, int n, int V, int k, int32_t *ids, float *weights, hipStream_t s) {
    if (!w || !ids || !weights || n <= 0 || V <= 0 || V >= (1 << 24) || k < 1 || k > SPARSE_MAX_K) return false;
    BERT_LAUNCH(sparse_topk_kernel, dim3((unsigned)n), dim3(256), 0, s, w, V, k, ids, weights);
    return true;
}

}  // namespace bert_hip
