// gemm_mx.hip — the MXFP8 forward route's mat-muls (BERT_HIP_MX=fp8; reference ops as gemm.hip: bert.cpp:822-839, :859-865, :878-891):
//   C[t][n] = epilogue( sum_k Aq[t][k] * Wq[n][k] + bias[n] (+ resid[t][n]) )
// on v_mfma_scale_f32_32x32x64_f8f6f4 with BOTH operands as MX rows (kernels.h: e4m3 codes, one E8M0 scale byte per 32 k), and the row
// quantiser that makes such rows of f16 activations.  The shape of the work:
//   * 128 features x 256 tokens per workgroup of 8 waves; a wave owns 64 features x 64 tokens = 2 x 2 accumulator blocks (64 registers:
//     the epilogue, which also quantises, has room);
//   * a reduction tile is 128 k: the weight tile (128 rows) and the activation tile (256 rows) are 18 + 36 KiB that lie in memory EXACTLY
//     as they lie in LDS — rows of 144 bytes = 128 codes, 4 scale bytes, 12 spare — so the tile load is 54 lane-linear 1 KiB pieces of
//     global_load_lds_dwordx4 with no address arithmetic per lane and no swizzle: nine 16-byte slots per row, an odd number, already put
//     the fragment reads of eight consecutive rows into eight different slots.  Two stages (108 KiB), one barrier per reduction tile;
//   * the main loop is 16 ds_read_b128, 4 ds_read_b32 and 8 MFMAs per wave and reduction tile, nothing else: no conversion, no scale
//     arithmetic.  The scale bytes ride in their row: a lane reads its row's scale dword, shifts it by 8 h once per tile, and byte 0 /
//     byte 2 (opsel 0 / 2) are the scales of the lane's k-blocks in the tile's two MFMA steps (the map ScoreBlock<mxfp4_t> verified);
//   * the tile is computed TRANSPOSED: the weights are the A operand, so an accumulator block's rows are features and its columns
//     tokens, and lane (col, h) holds features 8 g + 4 h + {0..3} of token col: the 32 consecutive features of one MX block of the
//     OUTPUT sit in lanes l and l ^ 32.  The MX output form — the f16 form followed by the row quantiser, bit for bit — is then 15
//     in-lane maxima, one v_permlane32_swap, and four dword stores of codes per block and lane;
//   * the f16 output form goes through a wave-private staging area (the dead stages) so that every global store is 16 bytes of a full
//     128-byte row segment, as gemm256.hip does it.
#include "device.h"

namespace bert_hip {

namespace {

constexpr int MX_BN = 128, MX_BM = 256;
constexpr int MX_A_BYTES = MX_BN * MX_ROW_BYTES, MX_B_BYTES = MX_BM * MX_ROW_BYTES;       // 18 KiB, 36 KiB
constexpr int MX_STAGE = MX_A_BYTES + MX_B_BYTES, MX_PIECES = MX_STAGE / 1024;           // 54 pieces of 1 KiB
constexpr int MX_STG_ROW = 144, MX_STG = 64 * MX_STG_ROW;                                // staging: 64 tokens x (64 halves + 16 bytes)
static_assert(MX_STAGE % 1024 == 0 && MX_A_BYTES % 1024 == 0, "a tile is whole 1 KiB pieces");
static_assert(8 * MX_STG <= 2 * MX_STAGE, "the staging areas lie in the dead stages");

struct GemmMxArgs {
    const uint8_t *w;        // GemmWeight::mx
    const uint8_t *a;        // MxRows of the activations, [KT][M_pad][144]
    const float *bias;       // [N]
    const half_t *resid;     // [M_pad][N] or null
    half_t *c16;             // [M_pad][N]                     (f16 form)
    uint8_t *cmx;            // MxRows [N / 128][M_pad][144]   (MX form)
    int N, M_pad, KT, n_tiles_n, n_items;
};

// ---- the MX block rule on a block's largest magnitude, as bits (an integer maximum: NaN > inf > every finite value, where fmaxf
// drops a NaN): the scale byte, 2^-e for the codes, and whether the block holds a non-finite value (kernels.h: zero codes under 0xFF)
struct MxBlockScale {
    float inv;
    uint32_t byte;
    bool bad;
    __device__ __forceinline__ explicit MxBlockScale(uint32_t amax_bits) {
        const int E = (int)(amax_bits >> 23);
        const int e = amax_bits == 0u ? 0 : max(E - 127 - 8, -127);
        bad = E == 255;
        inv = __builtin_bit_cast(float, (uint32_t)(127 - e) << 23);
        byte = bad ? 0xffu : (uint32_t)(e + 127);
    }
    // four values -> four e4m3 code bytes, the first in the low byte (device.h e4m3_code: the index quantiser's codes)
    __device__ __forceinline__ uint32_t codes(float v0, float v1, float v2, float v3) const {
        const float v[4] = {v0, v1, v2, v3};
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = v[j] * inv;                       // exact: a power of two, no result below f32's normals
            w |= ((__builtin_bit_cast(uint32_t, y) >> 31) << 7 | e4m3_code(fabsf(y))) << (8 * j);
        }
        return bad ? 0u : w;
    }
};
__device__ __forceinline__ uint32_t abs_bits(float v) { return __builtin_bit_cast(uint32_t, v) & 0x7fffffffu; }
// the maximum over the four lanes of a quad (quad_max_f32's two DPP steps on integers)
__device__ __forceinline__ uint32_t quad_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));
    return v;
}

template <int OFF>
__device__ __forceinline__ uint32_t lds_read_b32(unsigned addr) {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}

// the fragments of one reduction tile: [MFMA step][block][16-byte half] of the weight rows (a) and the token rows (b), the rows' scale dwords
struct MxFrag {
    i32x4 a[2][2][2], b[2][2][2];
    uint32_t sa[2], sb[2];
};
// hand-issued reads (device.h): the waits name what they release.  N: reads that may still be in flight
template <int N, int s>
__device__ __forceinline__ void mx_wait_step(MxFrag &f) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(f.a[s][0][0]), "+v"(f.a[s][0][1]), "+v"(f.a[s][1][0]), "+v"(f.a[s][1][1]), "+v"(f.b[s][0][0]), "+v"(f.b[s][0][1]),
                   "+v"(f.b[s][1][0]), "+v"(f.b[s][1][1])
                 : "n"(N) : "memory");
}

// tanh-form GELU in f32 (gemm.hip's): x / (1 + exp2(x (c1 + c2 x^2)))
__device__ __forceinline__ float mx_gelu(float x) {
    const float c1 = -2.0f * 0.79788456080286535588f * 1.44269504088896340736f;
    const float c2 = c1 * 0.044715f;
    const float t = x * __builtin_fmaf(x * x, c2, c1);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}
// One output value: f32 sum + bias (+ residual), GELU, ONE rounding to f16.  Both output forms call this and nothing else, and the
// result is materialised in f32 before the conversion (device.h rounded_f32): the MX form must quantise the f16 form's very bits.
template <int EPI>
__device__ __forceinline__ _Float16 mx_epi_value(float acc, float bias, float resid) {
    float v = acc + bias;
    if (EPI == EPI_BIAS_RESID) v = rounded_f32(v) + resid;
    if (EPI == EPI_BIAS_GELU) v = mx_gelu(rounded_f32(v));
    return (_Float16)rounded_f32(v);
}

}  // namespace

// f16 rows -> MX rows (kernels.h launch_mx_quantize_rows): a wave per row, a lane per 8 consecutive k of every 512, four lanes a block.
__global__ __launch_bounds__(256) void mx_quantize_rows_kernel(const half_t *__restrict__ x, int T, int K, uint8_t *__restrict__ out, int M_pad) {
    const int lane = threadIdx.x & 63, row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (row >= M_pad) return;
    const int K_pad = mx_k_tiles(K) * MX_K_TILE;
    for (int c0 = 8 * lane; c0 < K_pad; c0 += 512) {          // (whole quads: K_pad is a multiple of 128)
        f16x8 hv = {};
        if (row < T && c0 < K) hv = *(const f16x8 *)(x + (size_t)row * K + c0);
        float v[8];
        uint32_t m = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[j] = (float)hv[j]; m = max(m, abs_bits(v[j])); }
        const MxBlockScale sc(quad_max_u32(m));
        uint8_t *dst = out + ((size_t)(c0 >> 7) * M_pad + row) * MX_ROW_BYTES;
        *(uint2 *)(dst + (c0 & 127)) = make_uint2(sc.codes(v[0], v[1], v[2], v[3]), sc.codes(v[4], v[5], v[6], v[7]));
        if ((lane & 3) == 0) dst[MX_K_TILE + ((c0 & 127) >> 5)] = (uint8_t)sc.byte;
        if ((c0 & 127) == 0) { uint32_t *z = (uint32_t *)(dst + MX_K_TILE + 4); z[0] = z[1] = z[2] = 0u; }
    }
}

template <int EPI, bool MXOUT>
__global__ __launch_bounds__(512) void gemm_mx_kernel(GemmMxArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int item = xcd_item();                 // (kernels.h: the feature tiles of a token tile go to one XCD, which fetches that tile once)
    if (item >= p.n_items) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 7;
    const int wf = wave & 1, wq = wave >> 1;     // feature half (64) / token quarter (64) of the tile
    const int col = lane & 31, h = lane >> 5;
    const int nt = item % p.n_tiles_n, n0 = nt * MX_BN, m0 = (item / p.n_tiles_n) * MX_BM, KT = p.KT, N = p.N;

    // ---- LDS-DMA: a stage is 54 pieces of 1 KiB, piece q at q KiB of the stage: the weight tile's 18, then the activation tile's 36;
    // wave w issues pieces w, w + 8, ..  Both tiles are contiguous in memory (kernels.h), a lane's source is piece + 16 lane.
    const uint8_t *wsrc = p.w + (size_t)nt * KT * MX_A_BYTES + lane * 16;
    const uint8_t *asrc = p.a + (size_t)m0 * MX_ROW_BYTES + lane * 16;
    const size_t a_step = (size_t)p.M_pad * MX_ROW_BYTES;
    auto request = [&](int kt) __attribute__((always_inline)) {
        char *stage = smem + (kt & 1) * MX_STAGE;
        const uint8_t *w = wsrc + (size_t)kt * MX_A_BYTES, *a = asrc + (size_t)kt * a_step;
        static_for<(MX_PIECES + 7) / 8>([&](auto i_tag) __attribute__((always_inline)) {
            const int q = wave + 8 * decltype(i_tag)::value;          // (wave-uniform)
            if (q < MX_PIECES) {
                const uint8_t *base = q < MX_A_BYTES / 1024 ? w : a - MX_A_BYTES;     // (a scalar select)
                __builtin_amdgcn_global_load_lds(AS_GLOBAL(base + q * 1024), AS_LDS(stage + q * 1024), 16, 0, 0);
            }
        });
    };

    // ---- fragment addresses (stage 0): lane (col, h) feeds an MFMA step row `col` of its block, bytes 16 h .. and 32 + 16 h .. of the
    // step's 64 (step s: + 64 s), and names the scale of k-block h of the step
    unsigned aW[2], aA[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        aW[i] = lds_addr(smem) + (unsigned)((wf * 64 + i * 32 + col) * MX_ROW_BYTES + 16 * h);
        aA[i] = lds_addr(smem) + (unsigned)(MX_A_BYTES + (wq * 64 + i * 32 + col) * MX_ROW_BYTES + 16 * h);
    }
    const unsigned sc_off = (unsigned)(MX_K_TILE - 16 * h), sc_shift = 8u * (unsigned)h;

    f32x16 acc[2][2];                            // [feature block][token block]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16)0.f;

    request(0);
    for (int kt = 0; kt < KT; ++kt) {
        // this wave's pieces of tile kt have landed and its reads of tile kt - 1 have returned; behind the barrier that holds for all
        // waves: tile kt is whole, and the stage of tile kt - 1 is free for tile kt + 1
        dma_barrier<0>();
        if (kt + 1 < KT) request(kt + 1);
        const unsigned so = (unsigned)((kt & 1) * MX_STAGE);
        MxFrag f;
#pragma unroll
        for (int i = 0; i < 2; ++i) { f.sa[i] = lds_read_b32<0>(aW[i] + so + sc_off); f.sb[i] = lds_read_b32<0>(aA[i] + so + sc_off); }
        static_for<2>([&](auto s_tag) __attribute__((always_inline)) {
            constexpr int s = decltype(s_tag)::value;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f.a[s][i][0] = lds_read_b128<false, 64 * s, i32x4>(aW[i] + so);
                f.a[s][i][1] = lds_read_b128<false, 64 * s + 32, i32x4>(aW[i] + so);
                f.b[s][i][0] = lds_read_b128<false, 64 * s, i32x4>(aA[i] + so);
                f.b[s][i][1] = lds_read_b128<false, 64 * s + 32, i32x4>(aA[i] + so);
            }
        });
        // (LDS reads return in order: behind all but the newest eight, the scale dwords and step 0's fragments are here)
        mx_wait_step<8, 0>(f);
        asm volatile("" : "+v"(f.sa[0]), "+v"(f.sa[1]), "+v"(f.sb[0]), "+v"(f.sb[1]));
#pragma unroll
        for (int i = 0; i < 2; ++i) { f.sa[i] >>= sc_shift; f.sb[i] >>= sc_shift; }
        // (the opsel is an immediate of the instruction: a compile-time loop)
        static_for<2>([&](auto s_tag) __attribute__((always_inline)) {
            constexpr int s = decltype(s_tag)::value;
            if constexpr (s == 1) {
                __builtin_amdgcn_sched_barrier(0);            // (step 1's wait stays behind step 0's MFMAs)
                mx_wait_step<0, 1>(f);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const i32x8 a8 = {f.a[s][i][0][0], f.a[s][i][0][1], f.a[s][i][0][2], f.a[s][i][0][3], f.a[s][i][1][0], f.a[s][i][1][1], f.a[s][i][1][2], f.a[s][i][1][3]};
                    const i32x8 b8 = {f.b[s][j][0][0], f.b[s][j][0][1], f.b[s][j][0][2], f.b[s][j][0][3], f.b[s][j][1][0], f.b[s][j][1][1], f.b[s][j][1][2], f.b[s][j][1][3]};
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc[i][j], 0, 0, 2 * s, (int)f.sa[i], 2 * s, (int)f.sb[j]);
                }
        });
    }
    // every wave has read its last fragments: the stages are dead (no request is in flight: the last tile asked for none)
    dma_barrier<0>();

    // ---- epilogue.  Block (i, j), register 4 g + e of lane (col, h): feature n0 + 64 wf + 32 i + 8 g + 4 h + e of token m0 + 64 wq + 32 j + col
    char *const stg = smem + wave * MX_STG;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int fb = n0 + wf * 64 + i * 32 + 4 * h, tok = m0 + wq * 64 + j * 32 + col;
            f16x4 hv[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 b = *(const f32x4 *)(p.bias + fb + 8 * g);
                f16x4 r = {};
                if (EPI == EPI_BIAS_RESID) r = *(const f16x4 *)(p.resid + (size_t)tok * N + fb + 8 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[g][e] = mx_epi_value<EPI>(acc[i][j][4 * g + e], b[e], (float)r[e]);
            }
            if constexpr (!MXOUT) {
#pragma unroll
                for (int g = 0; g < 4; ++g) *(uint2 *)(stg + (j * 32 + col) * MX_STG_ROW + (i * 32 + 8 * g + 4 * h) * 2) = __builtin_bit_cast(uint2, hv[g]);
            } else {
                // the block of 32 features of this token: this lane's 16 values and lane ^ 32's
                uint32_t m = 0;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) m = max(m, abs_bits((float)hv[g][e]));
                float ma = __builtin_bit_cast(float, m), mb = ma;
                xor32_pair(ma, mb);                            // (bits only: the swap moves registers)
                const MxBlockScale sc(max(__builtin_bit_cast(uint32_t, ma), __builtin_bit_cast(uint32_t, mb)));
                // the consumer's k-tile nt: these 128 features are one k-tile of the rows
                uint8_t *dst = p.cmx + ((size_t)nt * p.M_pad + tok) * MX_ROW_BYTES;
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *(uint32_t *)(dst + wf * 64 + i * 32 + 8 * g + 4 * h) = sc.codes((float)hv[g][0], (float)hv[g][1], (float)hv[g][2], (float)hv[g][3]);
                if (h == 0) dst[MX_K_TILE + wf * 2 + i] = (uint8_t)sc.byte;
                if (h == 1 && wf == 0 && i == 0) { uint32_t *z = (uint32_t *)(dst + MX_K_TILE + 4); z[0] = z[1] = z[2] = 0u; }
            }
        }
    if constexpr (!MXOUT) {
        // the wave's 64 tokens x 64 features, 16 bytes a lane: eight lanes store a token's 128-byte row segment
        half_t *crow = p.c16 + (size_t)(m0 + wq * 64) * N + n0 + wf * 64;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = it * 8 + (lane >> 3), ch = lane & 7;
            *(uint4 *)(crow + (size_t)row * N + ch * 8) = *(const uint4 *)(stg + row * MX_STG_ROW + ch * 16);
        }
    }
}

void launch_mx_quantize_rows(const half_t *x, int T, int T_pad, int K, MxRows out, hipStream_t stream) {
    BERT_LAUNCH(mx_quantize_rows_kernel, dim3((T_pad + 3) / 4), dim3(256), 0, stream, x, T, K, out.p, T_pad);
}

bool gemm_mx_supported(const GemmWeight &W, int M_pad) {
    return W.mx != nullptr && W.K % 64 == 0 && W.N % MX_BN == 0 && M_pad % MX_BM == 0 && M_pad > 0;
}

void launch_gemm_mx(const GemmWeight &W, const MxRows &A, const float *bias, const half_t *resid, half_t *C16, MxRows *Cmx, int M_pad,
                    int epilogue, hipStream_t stream) {
    GemmMxArgs a;
    a.w = W.mx; a.a = A.p; a.bias = bias; a.resid = resid; a.c16 = C16; a.cmx = Cmx ? Cmx->p : nullptr;
    a.N = W.N; a.M_pad = M_pad; a.KT = mx_k_tiles(W.K); a.n_tiles_n = W.N / MX_BN;
    a.n_items = a.n_tiles_n * (M_pad / MX_BM);
    const size_t lds = 2 * MX_STAGE;
    static DeviceFlags configured[6];
    auto go = [&](auto kernel, int slot) {
        configure_once(configured[slot], [&] { (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
        BERT_LAUNCH(kernel, dim3(xcd_grid(a.n_items)), dim3(512), lds, stream, a);
    };
    auto by_form = [&](auto epi_tag) {
        constexpr int E = decltype(epi_tag)::value;
        if (C16) go(gemm_mx_kernel<E, false>, 2 * E);
        if (Cmx) go(gemm_mx_kernel<E, true>, 2 * E + 1);
    };
    switch (epilogue) {
        case EPI_BIAS: by_form(std::integral_constant<int, EPI_BIAS>{}); break;
        case EPI_BIAS_GELU: by_form(std::integral_constant<int, EPI_BIAS_GELU>{}); break;
        default: by_form(std::integral_constant<int, EPI_BIAS_RESID>{}); break;
    }
}

}  // namespace bert_hip
