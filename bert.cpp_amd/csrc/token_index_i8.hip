// token_index_i8.hip — the device code of the token index's int8 form (gfx950; bert_hip.h "TOKEN INDEX, int8 form"): token rows as int8
// codes with one f32 scale per token, and their exact MaxSim top-k search on v_mfma_i32_32x32x32_i8.  token_index_kernels.h states the
// stored form and the arguments; the TokenIndex class (token_index.cpp) plans and orders the launches.
//
//   token_i8_quantize_kernel  f32 or f16 rows -> codes and scales, one wave per row: search.hip's index_quantize_kernel, word for word
//                   (f16 is converted exactly first).  Serves the adds and, with qcu, the queries of every search and rescore.
//   token_i8_scan_kernel  token_index_scan_kernel's structure (token_index.hip): one workgroup of four waves per (query, slice), the XCD
//                   map, a wave owns whole documents, TOKEN_ROUNDS / TOKEN_STEP_DOCS, the list in LDS with the threshold in registers,
//                   every barrier met by all four waves, the guards, and under MASKED the 64-bit step mask from live & allow.
//     Query.        Staged once in LDS: codes as rows of dpad + 16 bytes, the scales beside them.  A ds_read_b128 step reads the 16 bytes
//                   at 32 s + 16 h of row col; its lane groups (MI355X: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) hold 16
//                   rows of all 16 residues mod 16 at one h, the row stride is (dpad / 16 + 1) slots of 16 bytes — an odd number, dpad being a
//                   multiple of 32 —, so the 16 rows lie on the 16 distinct slots of the 256-byte bank row: no conflict.
//     Score.        dot_ij exact in i32 (the document block is the A operand straight from global memory: lane (col, h) feeds step s
//                   the 16 bytes at 32 s + 16 h of row j0 + col — ScoreBlock<int8_t>::run's k map).  acc[r] is document token
//                   j0 + (r & 3) + 8 (r >> 2) + 4 h against query token col: per block of 32 document tokens 16 conversions (exact:
//                   |dot| < 2^24), 16 multiplies by the token's scale and 16 maxima; the 16 scales of a lane are four runs of four
//                   consecutive floats at j0 + 8 g + 4 h, whose alignment nothing promises (a 4-byte aligned 16-byte load).  The maximum
//                   m_i over the document is multiplied ONCE by the query token's scale, and the products are added as the f16 scan adds
//                   its maxima: blocks of 32 through wave_sum_f32 with +0 in lanes 32 .. 63 and behind the query's end, the blocks'
//                   sums in ascending order from +0.
//     Non-finite.   fmaxf drops a NaN, so a NaN scale is looked for on its own: a document with one (the unsigned maximum of the scales'
//                   bits is above +inf's) scores nothing and is never pushed; a query with one gets the guards' lists.
//     LISTED.       A rescore: a slice is a range of positions of the query's candidate list, a wave's document id comes from the list;
//                   an id outside [0, n_docs) or a removed one is no candidate, a repeated id is pushed each time.  One wave still sees a
//                   whole document: the search's bits by construction.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "device.h"
#include "token_index_kernels.h"
#include "topk_select.h"

namespace bert_hip {

namespace {

constexpr int SENT_ID = INT_MAX;        // id of an empty list entry (score -inf), as in token_index.hip

static_assert(TOKEN_STEP_DOCS == 64, "the masked scan keeps a step's mask in one 64-bit word");

// four consecutive scales at any 4-byte aligned address
struct __attribute__((aligned(4))) f32x4u { float v[4]; };

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
    const int dim = a.dim, dpad = a.dpad;
    const T *x = (const T *)a.src + row * dim;
    float amax = 0.f;
    int bad = 0;
    for (int c = lane; c < dim; c += 64) {
        const float v = (float)x[c];
        bad |= !__builtin_isfinite(v);                         // (fmaxf drops a NaN: tested on its own)
        amax = fmaxf(amax, fabsf(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    bad = __any(bad);
    const float scale = bad ? __builtin_nanf("") : amax / 127.0f;
    const bool zero = bad || scale == 0.f;
    if (lane == 0) a.scales[w] = scale;
    int8_t *out = a.codes + w * dpad;
    for (int c = 4 * lane; c < dpad; c += 256) {
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float v = c + j < dim ? (float)x[c + j] : 0.f;
            const float q = zero ? 0.f : fminf(fmaxf(__builtin_rintf(v / scale), -127.f), 127.f);
            packed |= (uint32_t)(uint8_t)(int8_t)(int)q << (8 * j);
        }
        *(uint32_t *)(out + c) = packed;
    }
}

// the word of live & allow (a null pointer: all ones) at index wi, the same in every lane
__device__ __forceinline__ uint32_t token_i8_mask_word(const TokenI8ScanArgs &a, int wi) {
    uint32_t w = ~0u;
    if (a.live) w &= a.live[wi];
    if (a.allow) w &= a.allow[wi];
    return __builtin_amdgcn_readfirstlane(w);
}

template <bool MASKED, bool LISTED>
__global__ __launch_bounds__(NT) void token_i8_scan_kernel(TokenI8ScanArgs a) {
    static_assert(!(MASKED && LISTED), "a rescore tests live per id");
    extern __shared__ __attribute__((aligned(16))) unsigned char t8_lds[];
    // (the XCD map of token_index_scan_kernel)
    const int item = (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8);
    if (item >= a.n_items) return;
    const int slice = item / a.nq, qi = item - slice * a.nq;
    const int P = a.dpad, ldq = P + 16, k = a.k, L = a.L;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, col = lane & 31, h = lane >> 5;
    int8_t *qs = (int8_t *)t8_lds;                                                         // [blocks of the launch][32][ldq]
    float *qsc = (float *)(t8_lds + (size_t)((a.max_q_len + TOKEN_QB - 1) / TOKEN_QB) * TOKEN_QB * ldq);       // [TOKEN_MAX_QUERY]
    float *ls = qsc + TOKEN_MAX_QUERY;
    int *li = (int *)(ls + L);
    int *cnt = li + L;
    // (everything up to the loop is uniform over the workgroup)
    const int q0 = a.qcu[qi], nq = a.qcu[qi + 1] - q0;
    const int n_list = LISTED ? a.n_cand : a.n_docs;           // what the slices cut: candidate positions, or documents
    const int r0 = (int)min((long long)slice * a.slice_docs, (long long)n_list);
    const int r1 = (int)min((long long)r0 + a.slice_docs, (long long)n_list);
    const size_t out = ((size_t)qi * a.n_slices + slice) * k;
    if (nq <= 0 || q0 < 0 || nq > a.max_q_len || r0 >= r1) {
        for (int j = tid; j < k; j += NT) { a.ws_s[out + j] = -INFINITY; a.ws_i[out + j] = SENT_ID; }
        return;
    }
    const int nblk = (nq + TOKEN_QB - 1) / TOKEN_QB, chunks = P >> 4;                      // (chunks: 16-byte pieces of a row)
    const i32x4 z = {};
    const int8_t *qsrc = a.q_codes + (size_t)qi * a.max_q_len * P;
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
    for (int i = tid; i < L; i += NT) { ls[i] = -INFINITY; li[i] = SENT_ID; }
    if (tid == 0) *cnt = 0;
    float ts = -INFINITY;
    int ti = SENT_ID;
    // a query with a non-finite token: the guards' lists (the barrier is the staging's)
    if (__syncthreads_or(qbad)) {
        for (int j = tid; j < k; j += NT) { a.ws_s[out + j] = -INFINITY; a.ws_i[out + j] = SENT_ID; }
        return;
    }

    const int room = L - k - TOKEN_STEP_DOCS;                  // a step pushes at most TOKEN_STEP_DOCS entries
    for (int base = r0; base < r1; base += TOKEN_STEP_DOCS) {
        // MASKED: token_index_scan_kernel's step mask, from the workgroup's values alone
        [[maybe_unused]] uint64_t m = 0;
        if constexpr (MASKED) {
            const int wi = base >> 5, sh = base & 31, we = (min(base + TOKEN_STEP_DOCS, r1) - 1) >> 5;
            const uint32_t w0 = token_i8_mask_word(a, wi);
            const uint32_t w1 = wi + 1 <= we ? token_i8_mask_word(a, wi + 1) : 0u;
            const uint32_t w2 = wi + 2 <= we ? token_i8_mask_word(a, wi + 2) : 0u;
            m = ((uint64_t)w1 << 32 | w0) >> sh;
            if (sh) m |= (uint64_t)w2 << (64 - sh);
            if (m == 0) continue;                              // (the whole workgroup: nothing was pushed)
        }
        for (int u = 0; u < TOKEN_ROUNDS; ++u) {
            const int pos = base + NWAVE * u + wave;           // (wave-uniform)
            if (pos >= r1) break;
            int d = pos;
            if constexpr (MASKED) {
                if (!(m >> (NWAVE * u + wave) & 1)) continue;  // (inside the round loop: the wave meets the step's barriers)
            }
            if constexpr (LISTED) {
                d = __builtin_amdgcn_readfirstlane(a.cand[(size_t)qi * a.n_cand + pos]);
                if (d < 0 || d >= a.n_docs) continue;
                if (a.live && !(__builtin_amdgcn_readfirstlane(a.live[d >> 5]) >> (d & 31) & 1u)) continue;
            }
            const int d0 = __builtin_amdgcn_readfirstlane(a.cu[d]), nd = __builtin_amdgcn_readfirstlane(a.cu[d + 1]) - d0;
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
                    const int8_t *drow = a.codes + (size_t)(d0 + (dok ? j0 + col : 0)) * P + 16 * h;
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
            const bool dbad = __any(sbits > 0x7f800000u);
            if (lane == 0 && !dbad && better(total, d, ts, ti)) {
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

DeviceFlags g_token_i8_lds;

// rows per launch of the quantisation: 2^22 waves of 64 threads, far below the 2^32 a launch's thread count wraps at
constexpr long long QUANT_MAX_ROWS = 1ll << 22;

}  // namespace

void token_i8_kernels_init() {
    // (as token_index_kernels_init)
    configure_once(g_token_i8_lds, [] {
        bool ok = true;
        for (const void *f : {(const void *)token_i8_scan_kernel<false, false>, (const void *)token_i8_scan_kernel<true, false>,
                              (const void *)token_i8_scan_kernel<false, true>})
            ok = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOKEN_LDS_MAX) == hipSuccess && ok;
        if (!ok) (void)hipGetLastError();
    });
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

void launch_token_i8_scan(const TokenI8ScanArgs &a, hipStream_t s) {
    if (a.n_items <= 0) return;
    const int grid = (a.n_items + 7) / 8 * 8;                  // (the kernel's XCD map)
    const size_t lds = token_i8_scan_lds_bytes(a.dim, a.max_q_len, a.k);
    if (a.cand) BERT_LAUNCH((token_i8_scan_kernel<false, true>), dim3(grid), dim3(NT), lds, s, a);
    else if (a.live || a.allow) BERT_LAUNCH((token_i8_scan_kernel<true, false>), dim3(grid), dim3(NT), lds, s, a);
    else BERT_LAUNCH((token_i8_scan_kernel<false, false>), dim3(grid), dim3(NT), lds, s, a);
}

}  // namespace bert_hip
