// score_chain.h — the f16 inner-product chain of the embedding index (search.hip ScoreBlock<half_t>::run) and of the late-interaction
// kernel (maxsim.hip): ONE statement of it, so a (row, row) product has the same bits wherever it is computed.
#pragma once
#include "device.h"

namespace bert_hip {

// One 32 x 32 block of inner products on v_mfma_f32_32x32x16_f16: acc[r] += A row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) against B row
// (lane & 31), f32 accumulation, k ascending in steps of 16 up to dpad (a multiple of 8; a last half step is the loaders' to fill
// with zeros).  load_a(k, in) / load_b(k, in): this lane's eight elements k + 8 (lane >> 5) .. + 7 of its row of the operand, for
// the step that starts at k; in == false: a step behind dpad, never multiplied (the loader returns zeros without reading).
template <class LoadA, class LoadB>
__device__ __forceinline__ void score_chain_f16(LoadA &&load_a, LoadB &&load_b, int dpad, f32x16 &acc) {
    constexpr int U = 8;
    for (int k0 = 0; k0 < dpad; k0 += 16 * U) {
        f16x8 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = k0 + 16 * u < dpad;
            a[u] = load_a(k0 + 16 * u, in);
            b[u] = load_b(k0 + 16 * u, in);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k0 + 16 * u < dpad) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[u], b[u], acc, 0, 0, 0);
    }
}

// The same chain for a grid of blocks that share operands (sparse_vocab.hip): acc[b][s] is the block of A operand s against B operand b,
// NA x NB of them.  Every accumulator sees the k sequence of score_chain_f16 — steps of 16 ascending, the same `in` rule — and nothing of
// its neighbours, so a (row, row) product keeps the bits of the single-block statement.  load_a(s, k, in) / load_b(b, k, in) as above;
// B's elements of a group of steps are loaded ahead (they come from global memory), A's as they are used (from LDS).
template <int NA, int NB, class LoadA, class LoadB>
__device__ __forceinline__ void score_chain_f16_grid(LoadA &&load_a, LoadB &&load_b, int dpad, f32x16 (&acc)[NB][NA]) {
    constexpr int U = 4;
    for (int k0 = 0; k0 < dpad; k0 += 16 * U) {
        f16x8 b[NB][U];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int n = 0; n < NB; ++n) b[n][u] = load_b(n, k0 + 16 * u, k0 + 16 * u < dpad);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k0 + 16 * u < dpad) {
#pragma unroll
                for (int s = 0; s < NA; ++s) {
                    const f16x8 a = load_a(s, k0 + 16 * u, true);
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc[n][s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b[n][u], acc[n][s], 0, 0, 0);
                }
            }
    }
}

}  // namespace bert_hip
