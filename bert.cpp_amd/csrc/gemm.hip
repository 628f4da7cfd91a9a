// gemm.hip — weight mat-muls of the encoder layer for gfx950 (CDNA4):
//   C[t][n] = epilogue( sum_k A[t][k] * W[n][k] + bias[n] )        A: f16 activations, W: f16 / q4_0 / q4_1
//
// Replaces ggml_mul_mat(weight, cur) + ggml_add(ggml_repeat(bias)) [+ ggml_gelu | + residual add]
// at reference bert.cpp:822-839 (Q/K/V, fused here into one [3H,H] weight), :859-865 (attention
// output + residual), :878-882 (FFN up + GELU), :885-891 (FFN down + residual).
//
// Design (one 64-wide wavefront = one 64x64 output sub-tile):
//   * 128 tokens x 128 features per workgroup of 4 waves, reduction tile 64 = two q4 blocks.
//   * v_mfma_f32_32x32x16_f16 with the WEIGHT tile as the A operand and the ACTIVATION tile as the
//     B operand, so a lane's accumulator column is one token and its registers are 4-feature
//     runs: the epilogue packs 4 f16 per 8-byte store and bias / residual loads are 4-wide.
//   * activation tiles (and f16 weight tiles) go HBM -> LDS by global_load_lds_dwordx4 (no VGPR
//     round trip), double buffered, one barrier per reduction tile.  The LDS image is lane-linear
//     per wave instruction, so the bank swizzle is applied to the SOURCE address and again on the
//     fragment read (chunk ^ ((row >> 1) & 7)), which makes every ds_read_b128 conflict-free.
//   * q4_0 / q4_1 weights stay quantised in HBM (16 B of nibbles + one f16 scale [+ f16 min] per
//     32 weights, tile-contiguous so a tile is one coalesced 4 KiB read); each thread dequantises
//     one block per reduction tile in registers (v_perm_b32 builds 1024+q half pairs, packed f16
//     math applies (q-8)*d or q*d+m) and writes four swizzled 16-B chunks into the LDS tile.
#include "device.h"

#include <algorithm>
#include <cstdlib>

namespace bert_hip {

struct GemmArgs {
    const half_t *A;        // [M_pad][K]
    const half_t *w16;      // [N_pad][K]
    const uint4 *qs;
    const void *sc;
    const float *bias;      // [N]
    const half_t *resid;    // [M_pad][N] or null
    half_t *C;              // [M_pad][N]
    int N, K, n_tiles_n;
};

constexpr int TILE_BYTES = 128 * 128;        // 128 rows x 64 halfs
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // activation tile + weight tile

// One wave instruction moves 8 rows x 128 B; a wave moves 32 rows, the workgroup the 128-row tile.
__device__ __forceinline__ void dma_tile(const half_t *src, int ld, char *tile, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int g = wave * 4 + i;
        const int r = g * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        __builtin_amdgcn_global_load_lds(AS_GLOBAL(src + (size_t)r * ld + c * 8), AS_LDS(tile + g * 1024), 16, 0, 0);
    }
}

__device__ __forceinline__ float gelu_tanh(float x) {
    // 0.5 x (1 + tanh(u)) == x / (1 + exp(-2u)),  u = sqrt(2/pi) x (1 + 0.044715 x^2)
    // exp(-2u) = exp2(x * (c1 + c2 x^2)); one v_exp_f32 + one v_rcp_f32 per element.
    const float c1 = -2.0f * 0.79788456080286535588f * 1.44269504088896340736f;
    const float c2 = c1 * 0.044715f;
    const float t = x * __builtin_fmaf(x * x, c2, c1);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}

// Workgroups are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8, each with a private
// L2).  Remap so that every XCD walks a CONTIGUOUS range of logical tiles: all feature tiles of one
// token tile then run back to back on one XCD and the activation tile is fetched from HBM once
// instead of once per XCD.  Bijective for any grid size.
__device__ __forceinline__ int xcd_remap(int bid, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// q4: this thread's block (row, half kb of the reduction tile) expanded into four swizzled 16-byte chunks of the weight tile
template <int WT>
__device__ __forceinline__ void dequant_block_to_lds(const RawBlock &blk, char *tile, int row, int kb) {
    q4_expand_block<WT, false>(blk, [&](int c) __attribute__((always_inline)) { return tile + off64(row, kb * 4 + c); });
}

template <int WT, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_mfma_kernel(GemmArgs p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = lb % p.n_tiles_n, mt = lb / p.n_tiles_n;
    const int m0 = mt * GEMM_BM, n0 = nt * GEMM_BN;
    const int K = p.K, nk = K / GEMM_BK;
    const int wf = wave & 1, wt = wave >> 1;          // feature half / token half of the tile
    const int l31 = lane & 31, hi = lane >> 5;

    const half_t *Abase = p.A + (size_t)m0 * K;
    const half_t *Wbase = p.w16 + (size_t)n0 * K;
    const size_t qbase = (size_t)nt * nk * 256;       // blocks of this feature tile, [kt][row][2]

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    RawBlock qn = {};

    // ---- prologue: tile 0 -> stage 0
    dma_tile(Abase, K, smem, wave, lane);
    if (WT == GW_F16) {
        dma_tile(Wbase, K, smem + TILE_BYTES, wave, lane);
    } else {
        qn = q4_load_block<WT>(p.qs, p.sc, qbase + tid);
        dequant_block_to_lds<WT>(qn, smem + TILE_BYTES, tid >> 1, tid & 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        char *cur = smem + (kt & 1) * STAGE_BYTES;
        char *nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;
        const bool more = kt + 1 < nk;
        if (more) {   // issue the next tile's HBM traffic before touching the matrix cores
            dma_tile(Abase + (kt + 1) * GEMM_BK, K, nxt, wave, lane);
            if (WT == GW_F16) {
                dma_tile(Wbase + (kt + 1) * GEMM_BK, K, nxt + TILE_BYTES, wave, lane);
            } else {
                qn = q4_load_block<WT>(p.qs, p.sc, qbase + (size_t)(kt + 1) * 256 + tid);
            }
        }
        const char *At = cur, *Wt = cur + TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int c = kk * 2 + hi;
            f16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *(const f16x8 *)(Wt + off64(wf * 64 + i * 32 + l31, c));
                b[i] = *(const f16x8 *)(At + off64(wt * 64 + i * 32 + l31, c));
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (WT != GW_F16 && more) dequant_block_to_lds<WT>(qn, nxt + TILE_BYTES, tid >> 1, tid & 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- epilogue.  Accumulator layout: lane owns token column l31 and 4-feature register runs.
    // Stage the 128x128 f32 tile in LDS (16-B chunk index XOR (token & 31): conflict-free both ways),
    // then every wave-instruction writes two full 256-B output rows: 32 lanes x 4 features each.
    // (The last reduction tile ended with a barrier, so the staging buffers are free.)
    float *Cs = (float *)smem;                 // [128 tokens][32 chunks of 4 floats]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int tok = wt * 64 + j * 32 + l31;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int chunk = wf * 16 + i * 8 + g * 2 + hi;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e];
                *(f32x4 *)(Cs + tok * 128 + ((chunk ^ (tok & 31)) << 2)) = v;
            }
        }
    __syncthreads();
    const int chunk = tid & 31;
    const int f0 = n0 + chunk * 4;
    if (f0 < p.N) {
        const f32x4 bv = *(const f32x4 *)(p.bias + f0);
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const int tok = s * 8 + (tid >> 5);
            f32x4 v = *(const f32x4 *)(Cs + tok * 128 + ((chunk ^ (tok & 31)) << 2));
            const size_t off = ((size_t)m0 + tok) * p.N + f0;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bv[e];
            if (EPI == EPI_BIAS_GELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
            }
            if (EPI == EPI_BIAS_RESID) {
                const f16x4 rv = *(const f16x4 *)(p.resid + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
            }
            f16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (_Float16)v[e];
            *(f16x4 *)(p.C + off) = o;
        }
    }
}

template <int WT>
static void launch_wt(const GemmArgs &a, int grid, int epilogue, hipStream_t s) {
    switch (epilogue) {
        case EPI_BIAS: BERT_LAUNCH((gemm_mfma_kernel<WT, EPI_BIAS>), dim3(grid), dim3(256), 0, s, a); break;
        case EPI_BIAS_GELU: BERT_LAUNCH((gemm_mfma_kernel<WT, EPI_BIAS_GELU>), dim3(grid), dim3(256), 0, s, a); break;
        default: BERT_LAUNCH((gemm_mfma_kernel<WT, EPI_BIAS_RESID>), dim3(grid), dim3(256), 0, s, a); break;
    }
}

void launch_gemm_mfma(const GemmWeight &W, const half_t *A, const float *bias, const half_t *resid, half_t *C,
                      int M_pad, int epilogue, hipStream_t stream) {
    GemmArgs a;
    a.A = A; a.w16 = W.w16; a.qs = W.qs; a.sc = W.sc; a.bias = bias; a.resid = resid; a.C = C;
    a.N = W.N; a.K = W.K; a.n_tiles_n = W.N_pad / GEMM_BN;
    const int grid = a.n_tiles_n * (M_pad / GEMM_BM);
    if (W.type == GW_F16) launch_wt<GW_F16>(a, grid, epilogue, stream);
    else if (W.type == GW_Q4_0) launch_wt<GW_Q4_0>(a, grid, epilogue, stream);
    else launch_wt<GW_Q4_1>(a, grid, epilogue, stream);
}

// ------------------------------------------------------------------------------------------------
// generic fallback: one thread per output element, f16 weights [N][K] (dequantised copy)
// ------------------------------------------------------------------------------------------------
template <int EPI>
__global__ void gemm_naive_kernel(const half_t *A, const half_t *W, const float *bias, const half_t *resid, half_t *C,
                                  int M, int N, int K) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63);
    const int t = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (n >= N || t >= M) return;
    const half_t *a = A + (size_t)t * K, *w = W + (size_t)n * K;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += (float)a[k] * (float)w[k];
    s += bias[n];
    if (EPI == EPI_BIAS_GELU) s = gelu_tanh(s);
    if (EPI == EPI_BIAS_RESID) s += (float)resid[(size_t)t * N + n];
    C[(size_t)t * N + n] = (_Float16)s;
}

// grid.y counts groups of 4 token rows and a grid dimension holds 65535 (kernels.h GRID_YZ_MAX: the limit the code assumes of
// every device): a chunk of 262 144 tokens is 65 536 groups, so the rows go in slices of 4 * 65535.
void launch_gemm_naive(const GemmWeight &W, const half_t *A, const float *bias, const half_t *resid, half_t *C,
                       int M, int epilogue, hipStream_t stream) {
    for (int m0 = 0; m0 < M; m0 += 4 * GRID_YZ_MAX) {
        const int m = std::min(4 * GRID_YZ_MAX, M - m0);
        const dim3 grid((W.N + 63) / 64, (m + 3) / 4), block(256);
        const half_t *a = A + (size_t)m0 * W.K, *r = resid ? resid + (size_t)m0 * W.N : nullptr;
        half_t *c = C + (size_t)m0 * W.N;
        switch (epilogue) {
            case EPI_BIAS: BERT_LAUNCH((gemm_naive_kernel<EPI_BIAS>), grid, block, 0, stream, a, W.naive16, bias, r, c, m, W.N, W.K); break;
            case EPI_BIAS_GELU: BERT_LAUNCH((gemm_naive_kernel<EPI_BIAS_GELU>), grid, block, 0, stream, a, W.naive16, bias, r, c, m, W.N, W.K); break;
            default: BERT_LAUNCH((gemm_naive_kernel<EPI_BIAS_RESID>), grid, block, 0, stream, a, W.naive16, bias, r, c, m, W.N, W.K); break;
        }
    }
}

}  // namespace bert_hip
