// token_proj.hip — the projection head of a ColBERT checkpoint over the token rows of a pass (kernels.h launch_token_project):
//   out[t][p] = sum_k Wp[p][k] x[t][k],  optionally over the row's own L2 norm, f32 or f16,
// on v_mfma_f32_32x32x16_f16.  Wp [P][H] is small (P <= 256) and shared by everybody; x [T][H] is read once and is what the launch costs.
// The shape of the work:
//   * a workgroup of four waves serves 128 consecutive tokens; a wave owns 32 tokens and ALL P features: NB = P / 32 accumulator blocks
//     (at most 8: 128 registers).  Nothing is reduced across waves and no x row is read by two of them;
//   * the product is computed TRANSPOSED, as gemm_mx.hip does: Wp is the A operand, so an accumulator block's rows are features and its
//     columns tokens: lane (col, h) holds features 32 j + 8 g + 4 h + {0..3} (register 4 g + e of block j) of token col.  A token's P
//     features lie in lanes l and l ^ 32: the L2 norm is NB x 16 in-lane squares and one v_permlane32_swap, no LDS;
//   * x goes from global memory straight into registers: lane (col, h) asks for the 16 bytes k + 8 h .. of its token's row for the four
//     MFMA steps of the NEXT 64-wide k-tile in front of this tile's MFMAs (score_chain_f16_shared_a's precedent: an operand taken from
//     global memory a group of steps ahead).  Rows at or beyond T and k at or beyond H are zeros that are never read;
//   * Wp comes out of L2 in k-tiles of 64 through a two-stage LDS ring by global_load_lds_dwordx4.  A tile row is 144 bytes — 128 of
//     halves and 16 spare: nine 16-byte slots, an odd number, so the ds_read_b128 of 32 consecutive rows hit distinct slots —; piece q of
//     a stage (16 bytes at 16 q: LDS-DMA writes lane-linearly) is slot q % 9 of row q / 9, and the lanes of the ninth slot ask for
//     nothing.  A stage is P x 144 bytes: 36 KiB at P = 256.  Pieces of the last tile whose k is at or beyond H are written as zeros by
//     ds_write instead, so the loop multiplies zeros there.  One barrier per k-tile;
//   * a tile is 4 x NB ds_read_b128 and 4 x NB MFMAs per wave; the reads of step s + 1 are issued in front of the MFMAs of step s and
//     retired by a counted wait (device.h: hand-issued reads);
//   * epilogue, per accumulator block through a wave-private staging area in the dead ring (32 tokens x (32 values + 16 bytes)), so that
//     every global store is 16 bytes of a row segment: 128-byte segments of f32 rows, 64-byte segments of f16 rows.
// The norm, exactly (tests/token_proj_reference.py restates it): a lane adds the squares of its values, each product rounded to f32,
// in ascending feature order; the two lanes' sums are added (h = 0's first); scale = 1 / sqrtf(sum), no epsilon; value * scale.
#include "device.h"

namespace bert_hip {

namespace {

constexpr int TP_ROW = 144;                       // bytes of a ring row: 64 halves + 16
constexpr int TP_SLOTS = TP_ROW / 16;             // 9
constexpr int TP_STG_WAVE = 32 * TP_ROW;          // a wave's staging area: 32 tokens x (128 bytes of values + 16)

struct TokenProjectArgs {
    const half_t *x;         // [T][H]
    const half_t *wp;        // [P][H]
    const int32_t *cu;       // [n_sentences + 1]
    void *out;               // [T][P] f32 or f16
    int T, H, n_sentences, max_len, flags;
};

}  // namespace

template <int NB>
__global__ __launch_bounds__(256) void token_project_kernel(TokenProjectArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int P = 32 * NB, STAGE = P * TP_ROW, PIECES = P * TP_SLOTS, GROUPS = (PIECES + 63) / 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6) & 3;
    const int col = lane & 31, h = lane >> 5;
    const int T = p.T, H = p.H, KT = (H + 63) >> 6;
    const int tok = (int)blockIdx.x * 128 + wave * 32 + col;
    const bool live = tok < T;

    // ---- Wp tile kt -> stage kt & 1: wave w issues the 1 KiB groups w, w + 4, ..; lane-linear piece q = slot q % 9 of row q / 9
    auto request_w = [&](int kt) __attribute__((always_inline)) {
        char *stage = smem + (kt & 1) * STAGE;
        static_for<(GROUPS + 3) / 4>([&](auto i_tag) __attribute__((always_inline)) {
            const int grp = wave + 4 * decltype(i_tag)::value;            // (wave-uniform)
            if (grp < GROUPS) {
                const int q = grp * 64 + lane, row = q / TP_SLOTS, slot = q - row * TP_SLOTS, k = kt * 64 + slot * 8;
                if (q < PIECES && slot < 8) {
                    if (k < H) __builtin_amdgcn_global_load_lds(AS_GLOBAL(p.wp + (size_t)row * H + k), AS_LDS(stage + grp * 1024), 16, 0, 0);
                    else *(uint4 *)(stage + q * 16) = make_uint4(0u, 0u, 0u, 0u);
                }
            }
        });
    };
    // ---- this lane's x elements of tile kt: k = 64 kt + 16 s + 8 h .. + 7 of row tok, zeros where there is nothing to read
    const half_t *xrow = p.x + (size_t)(live ? tok : 0) * H + 8 * h;
    auto request_x = [&](int kt, f16x8 (&f)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kt * 64 + 16 * s;
            f[s] = (f16x8)(_Float16)0;
            if (live && k + 8 * h < H) f[s] = *(const f16x8 *)(xrow + k);
        }
    };

    f32x16 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = (f32x16)0.f;

    f16x8 xf[4], xn[4];
    request_w(0);
    request_x(0, xf);

    // ---- the guard (launch_token_rows' rule), under the first requests: the largest b with cu[b] <= tok, and whether tok is one of
    // the tokens of a sentence of 1 .. max_len tokens
    bool bad = true;
    if (live) {
        int lo = 0, hi = p.n_sentences;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (p.cu[mid] <= tok) lo = mid; else hi = mid;
        }
        const int c0 = p.cu[lo], c1 = p.cu[lo + 1], n = c1 - c0;
        bad = n < 1 || n > p.max_len || tok < c0 || tok >= c1;
    }

    // fragment address (stage 0): lane (col, h) feeds an MFMA step row col of its feature block, bytes 16 h .. of the step's 32
    const unsigned aW = lds_addr(smem) + (unsigned)(col * TP_ROW + 16 * h);
    for (int kt = 0; kt < KT; ++kt) {
        // this wave's pieces of tile kt have landed (and its x elements with them) and its reads of tile kt - 1 have returned; behind the
        // barrier that holds for all waves: tile kt is whole, and the stage of tile kt - 1 is free for tile kt + 1
        dma_barrier<0>();
        if (kt + 1 < KT) { request_w(kt + 1); request_x(kt + 1, xn); }
        const unsigned a0 = aW + (unsigned)((kt & 1) * STAGE);
        f16x8 w[2][NB];
        static_for<NB>([&](auto j_tag) __attribute__((always_inline)) {
            constexpr int j = decltype(j_tag)::value;
            w[0][j] = lds_read_b128<false, j * 32 * TP_ROW>(a0);
        });
        static_for<4>([&](auto s_tag) __attribute__((always_inline)) {
            constexpr int s = decltype(s_tag)::value;
            if constexpr (s < 3)
                static_for<NB>([&](auto j_tag) __attribute__((always_inline)) {
                    constexpr int j = decltype(j_tag)::value;
                    w[(s + 1) & 1][j] = lds_read_b128<false, j * 32 * TP_ROW + 32 * (s + 1)>(a0);
                });
            // (LDS reads return in order: behind all but the newest NB, step s's fragments are here)
            asm volatile("s_waitcnt lgkmcnt(%0)" : : "n"(s < 3 ? NB : 0) : "memory");
#pragma unroll
            for (int j = 0; j < NB; ++j) landed(w[s & 1][j]);
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[s & 1][j], xf[s], acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                 // (the next step's reads stay behind this step's wait)
        });
        if (kt + 1 < KT) {
#pragma unroll
            for (int s = 0; s < 4; ++s) xf[s] = xn[s];
        }
    }
    // every wave has read its last fragments: the stages are dead (no request is in flight: the last tile asked for none)
    dma_barrier<0>();

    // ---- epilogue.  Register 4 g + e of block j in lane (col, h): feature 32 j + 8 g + 4 h + e of token tok
    const bool norm = p.flags & TOKEN_ROWS_NORMALIZE, o16 = p.flags & TOKEN_ROWS_F16;
    float scale = 1.f;
    if (norm) {
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) sq = sq + rounded_f32(acc[j][r] * acc[j][r]);       // (two roundings: never an fma)
        float s0 = sq, s1 = sq;
        xor32_pair(s0, s1);
        scale = 1.0f / sqrtf(s0 + s1);                         // (xor32_pair: s0 is h = 0's sum in both halves)
    }
    const float nan = __builtin_nanf("");
    char *const stg = smem + wave * TP_STG_WAVE;
    const int tok0 = (int)blockIdx.x * 128 + wave * 32;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        if (o16) {
            // rows of 32 halves + 16 bytes (80: five slots, odd); 8 bytes a lane and g
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (_Float16)rounded_f32(bad ? nan : acc[j][4 * g + e] * scale);
                *(uint2 *)(stg + col * 80 + (8 * g + 4 * h) * 2) = __builtin_bit_cast(uint2, hv);
            }
            // 16 tokens an instruction, four lanes a token's 64-byte segment
            half_t *orow = (half_t *)p.out + (size_t)tok0 * P + 32 * j;
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int row = it * 16 + (lane >> 2), ch = lane & 3;
                const uint4 v = *(const uint4 *)(stg + row * 80 + ch * 16);
                if (tok0 + row < T) *(uint4 *)(orow + (size_t)row * P + ch * 8) = v;
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = bad ? nan : acc[j][4 * g + e] * scale;
                *(f32x4 *)(stg + col * TP_ROW + (8 * g + 4 * h) * 4) = v;
            }
            // 8 tokens an instruction, eight lanes a token's 128-byte segment
            float *orow = (float *)p.out + (size_t)tok0 * P + 32 * j;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                const uint4 v = *(const uint4 *)(stg + row * TP_ROW + ch * 16);
                if (tok0 + row < T) *(uint4 *)(orow + (size_t)row * P + ch * 4) = v;
            }
        }
    }
}

bool token_project_supported(int H, int P) { return H >= 8 && H % 8 == 0 && P >= 32 && P <= TOKEN_PROJ_MAX_P && P % 32 == 0; }

void launch_token_project(const half_t *x, const half_t *wp, int T, int H, int P, const int32_t *cu_seqlens, int n_sentences, int max_len,
                          int flags, void *out, hipStream_t stream) {
    if (T <= 0 || n_sentences <= 0 || !token_project_supported(H, P)) return;
    const TokenProjectArgs a{x, wp, cu_seqlens, out, T, H, n_sentences, max_len, flags};
    const int nb = P / 32;
    // the ring, or the four staging areas where two stages are smaller
    const size_t lds = std::max<size_t>(2 * (size_t)P * TP_ROW, 4 * (size_t)TP_STG_WAVE);
    static DeviceFlags configured[8];
    auto go = [&](auto kernel) {
        configure_once(configured[nb - 1], [&] { (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); });
        BERT_LAUNCH(kernel, dim3((T + 127) / 128), dim3(256), lds, stream, a);
    };
    switch (nb) {
        case 1: go(token_project_kernel<1>); break;
        case 2: go(token_project_kernel<2>); break;
        case 3: go(token_project_kernel<3>); break;
        case 4: go(token_project_kernel<4>); break;
        case 5: go(token_project_kernel<5>); break;
        case 6: go(token_project_kernel<6>); break;
        case 7: go(token_project_kernel<7>); break;
        default: go(token_project_kernel<8>); break;
    }
}

}  // namespace bert_hip
