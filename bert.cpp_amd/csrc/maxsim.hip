// maxsim.hip — late-interaction (MaxSim) scoring of two packed sets of f16 token rows (gfx950; bert_hip.h "token rows and late
// interaction"): score(a, b) = sum over the tokens i of query sentence a of ( max over the tokens j of document sentence b of
// <Q_i, D_j> ), divided by (float)len(a) with mode bit 0.
//
//   maxsim_kernel   one workgroup of 4 waves per pair.  The pair's query tokens go in blocks of 32; a block is staged once in LDS
//                   (32 rows of H + 8 halfs: the 16 bytes of padding put the 32 rows a ds_read_b128 step touches on distinct
//                   bank groups).  Wave w takes the document's 32-token blocks w, w + 4, ... straight from global memory / L2
//                   as the index kernels take their rows, runs score_chain_f16 (score_chain.h: ScoreBlock<half_t>::run's chain)
//                   with the document block as the A operand and the query block as the B operand — lane (c, h) then holds
//                   query token c against document tokens (r & 3) + 8 (r >> 2) + 4 h in accumulator register r — and keeps a
//                   running elementwise max of the 16 registers over its blocks.  At the end of the query block a lane folds its
//                   16 maxima, meets lane ^ 32 (xor32_max), the four waves' 32 maxima meet in LDS, and wave 0 sums them.
//   Masking.        A document slot at or behind len(b) enters the max as -inf (its operand is zero-filled, never read, and the
//                   product 0 it gives is replaced before the max); a wave without a block keeps -inf.  A query slot at or behind
//                   len(a) adds +0 to the sum.  Rows outside the pair's two ranges are never read.
//   Order.          The max is exact (no rounding; fmaxf drops a NaN product, so a NaN element hides its token instead of the pair).
//                   The sum: per query block, lane c < 32 of wave 0 holds token c's maximum (lanes 32 .. 63 and slots behind len(a)
//                   hold +0), wave_sum_f32 adds the 64 lanes in its fixed butterfly order; the blocks' sums are added in ascending
//                   block order to a total that starts at +0; the mean is one division by (float)len(a).  No atomics, nothing
//                   depends on the grid: a pair's bits depend on its own rows alone.
//   Errors.         A pair index outside [0, n_q) x [0, n_d), or a sentence whose cu entries do not ascend strictly (empty or
//                   descending) or start below 0: that pair's score is NaN, nothing else is touched.
//   f32_to_f16_kernel  the host form's rows, rounded to nearest even.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "device.h"
#include "score_chain.h"

namespace bert_hip {

namespace {

constexpr int MS_WAVES = 4, MS_NT = 64 * MS_WAVES, MS_QB = 32;

__global__ __launch_bounds__(MS_NT) void maxsim_kernel(MaxsimArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ms_lds[];
    const int H = a.H, ldq = H + 8;                            // (halfs per staged row)
    half_t *qs = (half_t *)ms_lds;                             // [MS_QB][ldq]
    float *wmax = (float *)(ms_lds + (size_t)MS_QB * ldq * 2); // [MS_WAVES][32]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, col = lane & 31, h = lane >> 5;
    const long long p = a.first + blockIdx.x;
    int pa, pb;
    if (a.pairs) { pa = a.pairs[2 * p]; pb = a.pairs[2 * p + 1]; }
    else { pa = (int)(p / a.n_d); pb = (int)(p - (long long)pa * a.n_d); }
    int q0 = 0, nq = 0, d0 = 0, nd = 0;
    if (pa >= 0 && pa < a.n_q && pb >= 0 && pb < a.n_d) {
        q0 = a.qcu[pa]; nq = a.qcu[pa + 1] - q0;
        d0 = a.dcu[pb]; nd = a.dcu[pb + 1] - d0;
    }
    if (nq <= 0 || nd <= 0 || q0 < 0 || d0 < 0) {              // (uniform: the whole workgroup leaves)
        if (tid == 0) a.scores[p] = __builtin_nanf("");
        return;
    }
    const int chunks = H >> 3;                                 // 16-byte pieces of a row
    const f16x8 z = {};
    float total = 0.f;
    for (int qb = 0; qb < nq; qb += MS_QB) {
        const int nrows = min(MS_QB, nq - qb);
        __syncthreads();                                       // (the block before: every wave has read its rows and wmax)
        for (int i = tid; i < nrows * chunks; i += MS_NT) {
            const int r = i / chunks, c = i - r * chunks;
            *(f16x8 *)(qs + r * ldq + 8 * c) = *(const f16x8 *)(a.q + (size_t)(q0 + qb + r) * H + 8 * c);
        }
        __syncthreads();
        const bool qok = col < nrows;
        const half_t *qrow = qs + col * ldq;
        f32x16 m;
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
        for (int blk = wave; blk * 32 < nd; blk += MS_WAVES) {
            const int j0 = blk * 32;
            const bool dok = j0 + col < nd;                    // this lane's row of the A operand: document token j0 + col
            const half_t *drow = a.d + (size_t)(d0 + (dok ? j0 + col : 0)) * H;
            f32x16 acc = {};
            score_chain_f16([&](int k, bool in) __attribute__((always_inline)) { return dok && in && k + 8 * h < H ? *(const f16x8 *)(drow + k + 8 * h) : z; },
                            [&](int k, bool in) __attribute__((always_inline)) { return qok && in && k + 8 * h < H ? *(const f16x8 *)(qrow + k + 8 * h) : z; },
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
        if (h == 0) wmax[wave * 32 + col] = v;
        __syncthreads();
        if (wave == 0) {
            float c = 0.f;
            if (h == 0 && qok) c = __builtin_fmaxf(__builtin_fmaxf(wmax[col], wmax[32 + col]), __builtin_fmaxf(wmax[64 + col], wmax[96 + col]));
            total += wave_sum_f32(c);
        }
    }
    if (tid == 0) a.scores[p] = (a.mode & 1) ? total / (float)nq : total;
}

__global__ __launch_bounds__(256) void f32_to_f16_kernel(const float *__restrict__ src, half_t *__restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (_Float16)src[i];
}

DeviceFlags g_maxsim_configured;

}  // namespace

size_t maxsim_lds_bytes(int H) { return (size_t)MS_QB * (H + 8) * 2 + MS_WAVES * 32 * sizeof(float); }

void launch_maxsim(const MaxsimArgs &a, hipStream_t s, int launch_pairs) {
    const long long n = a.pairs ? a.n_pairs : (long long)a.n_q * a.n_d;
    if (n <= 0) return;
    // (a grid of 2^32 threads or more is not run as asked: at most 2^31 per launch)
    const long long per = launch_pairs >= 1 && launch_pairs < MAXSIM_LAUNCH_PAIRS ? launch_pairs : MAXSIM_LAUNCH_PAIRS;
    // (H = 1024 needs 66 560 bytes: past the 64 KiB a kernel gets without asking)
    configure_once(g_maxsim_configured, [] { (void)hipFuncSetAttribute((const void *)maxsim_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxsim_lds_bytes(MAXSIM_MAX_H)); });
    MaxsimArgs part = a;
    for (part.first = 0; part.first < n; part.first += per)
        BERT_LAUNCH(maxsim_kernel, dim3((unsigned)std::min(per, n - part.first)), dim3(MS_NT), maxsim_lds_bytes(a.H), s, part);
}

void launch_f32_to_f16(const float *src, half_t *dst, size_t n, hipStream_t s) {
    if (!n) return;                                            // (n <= F32_TO_F16_MAX_N: kernels.h)
    BERT_LAUNCH(f32_to_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
}

}  // namespace bert_hip
