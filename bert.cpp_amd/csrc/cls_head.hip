// cls_head.hip — the classification head of a cross-encoder (gfx950; bert_hip.h "sentence pairs and scores"): from the un-normalised
// [CLS] rows of a pass, f32 [B][H], to out[b][l] = bc[l] + sum_f Wc[l][f] tanh(bp[f] + <Wp[f], row_b>), f32 [B][n_labels]
// (BertForSequenceClassification: pooler, then classifier; no dropout at inference).
//
//   cls_head_kernel      the matrix-core form, H % 8 == 0, H <= 1024.  The pooler is the index's problem with the roles named anew: the
//                        H rows of Wp are the "index rows", a block of 32 sentences the "queries".  A workgroup of 4 waves owns 32
//                        sentences and stages their rows once, rounded to f16, in LDS (32 rows of H + 8 halfs: maxsim.hip's padding);
//                        a slot behind B is staged as zeros, never read from memory and never stored.  Wave w takes the feature blocks
//                        w, w + 4, ... of 32 features each; Wp's rows go from L2 straight to registers as the A operand of
//                        score_chain_f16 (score_chain.h), the staged rows are the B operand: lane (c, h) then holds sentence c against
//                        features f0 + (r & 3) + 8 (r >> 2) + 4 h in accumulator register r.  The epilogue stays in registers: + bp,
//                        tanhf, times the lane's Wc[l][feature] for each label.
//   Order.               Per feature block and label a lane adds its 16 products in ascending r by an fmaf chain from +0, the two
//                        lane halves meet (xor32_sum), and the block's sum joins the wave's running logit: blocks in ascending order.
//                        The four waves' logits meet in LDS as (w0 + w1) + (w2 + w3); bc is added last.  No atomics, nothing depends
//                        on the grid or on the other columns of the matrix-core block: a sentence's bits depend on its own row alone
//                        — the same alone, anywhere in a batch, in any batch size.
//   cls_head_f32_kernel  the plain form: one workgroup of 4 waves per sentence, the row in LDS as f32.  Wave w takes the features w,
//                        w + 4, ...: a lane's fmaf chain over k = lane, lane + 64, ..., wave_sum_f32, + bp, tanhf -> LDS.  Then wave w
//                        takes the labels w, w + 4: the same chain over the pooled features, + bc.  W: Wp as f32 (the f32 route: f32
//                        files under f32_exact) or f16 (any H the matrix-core form refuses).
//   Flags.               bit 0: 1 / (1 + expf(-logit)) per label instead of the logit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "device.h"
#include "score_chain.h"

namespace bert_hip {

namespace {

constexpr int CH_WAVES = 4, CH_NT = 64 * CH_WAVES, CH_SB = 32, CH_NL = CLS_HEAD_MAX_LABELS;

__device__ __forceinline__ float cls_head_out(float logit, int flags) { return (flags & CLS_HEAD_SIGMOID) ? 1.0f / (1.0f + expf(-logit)) : logit; }

__global__ __launch_bounds__(CH_NT) void cls_head_kernel(ClsHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ch_lds[];
    const int H = a.H, NL = a.n_labels, ld = H + 8;            // (halfs per staged row)
    half_t *rs = (half_t *)ch_lds;                             // [CH_SB][ld]
    float *wsum = (float *)(ch_lds + (size_t)CH_SB * ld * 2);  // [CH_WAVES][CH_NL][32]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, col = lane & 31, h = lane >> 5;
    const int s0 = blockIdx.x * CH_SB, nrows = min(CH_SB, a.B - s0);
    const int chunks = H >> 3;                                 // 8-element pieces of a row
    for (int i = tid; i < CH_SB * chunks; i += CH_NT) {
        const int r = i / chunks, c = i - r * chunks;
        f16x8 v = {};
        if (r < nrows) {
            const float *src = a.rows + (size_t)(s0 + r) * H + 8 * c;
            const float4 x = *(const float4 *)src, y = *(const float4 *)(src + 4);
            v = f16x8{(_Float16)x.x, (_Float16)x.y, (_Float16)x.z, (_Float16)x.w, (_Float16)y.x, (_Float16)y.y, (_Float16)y.z, (_Float16)y.w};
        }
        *(f16x8 *)(rs + r * ld + 8 * c) = v;
    }
    __syncthreads();
    const half_t *srow = rs + col * ld;
    const f16x8 z = {};
    float logit[CH_NL];
#pragma unroll
    for (int l = 0; l < CH_NL; ++l) logit[l] = 0.f;
    for (int f0 = wave * 32; f0 < H; f0 += 32 * CH_WAVES) {
        const bool fok = f0 + col < H;                         // this lane's row of the A operand: feature f0 + col
        const half_t *wrow = a.wp16 + (size_t)(fok ? f0 + col : 0) * H;
        f32x16 acc = {};
        score_chain_f16([&](int k, bool in) __attribute__((always_inline)) { return fok && in && k + 8 * h < H ? *(const f16x8 *)(wrow + k + 8 * h) : z; },
                        [&](int k, bool in) __attribute__((always_inline)) { return in && k + 8 * h < H ? *(const f16x8 *)(srow + k + 8 * h) : z; },
                        H, acc);
        float part[CH_NL];
#pragma unroll
        for (int l = 0; l < CH_NL; ++l) part[l] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = f0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (f < H) {
                const float p = tanhf(acc[r] + a.bp[f]);
#pragma unroll
                for (int l = 0; l < CH_NL; ++l)
                    if (l < NL) part[l] = fmaf(p, a.wc[(size_t)l * H + f], part[l]);
            }
        }
#pragma unroll
        for (int l = 0; l < CH_NL; ++l)
            if (l < NL) logit[l] += xor32_sum(part[l]);
    }
#pragma unroll
    for (int l = 0; l < CH_NL; ++l)
        if (l < NL && h == 0) wsum[(wave * CH_NL + l) * 32 + col] = logit[l];
    __syncthreads();
    // thread (label tid >> 5, sentence tid & 31): CH_NL x 32 = CH_NT of them
    const int l = tid >> 5, c = tid & 31;
    if (l < NL && c < nrows) {
        const float v = ((wsum[(0 * CH_NL + l) * 32 + c] + wsum[(1 * CH_NL + l) * 32 + c]) + (wsum[(2 * CH_NL + l) * 32 + c] + wsum[(3 * CH_NL + l) * 32 + c])) + a.bc[l];
        a.out[(size_t)(s0 + c) * NL + l] = cls_head_out(v, a.flags);
    }
}

template <class W>
__global__ __launch_bounds__(CH_NT) void cls_head_f32_kernel(ClsHeadArgs a, const W *__restrict__ wp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ch_lds[];
    const int H = a.H, NL = a.n_labels;
    float *row = (float *)ch_lds, *pooled = row + H;           // [H], [H]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int b = blockIdx.x;
    for (int e = tid; e < H; e += CH_NT) row[e] = a.rows[(size_t)b * H + e];
    __syncthreads();
    for (int f = wave; f < H; f += CH_WAVES) {
        const W *w = wp + (size_t)f * H;
        float s = 0.f;
        for (int k = lane; k < H; k += 64) s = fmaf(row[k], (float)w[k], s);
        s = wave_sum_f32(s);
        if (lane == 0) pooled[f] = tanhf(s + a.bp[f]);
    }
    __syncthreads();
    for (int l = wave; l < NL; l += CH_WAVES) {
        const float *w = a.wc + (size_t)l * H;
        float s = 0.f;
        for (int k = lane; k < H; k += 64) s = fmaf(pooled[k], w[k], s);
        s = wave_sum_f32(s);
        if (lane == 0) a.out[(size_t)b * NL + l] = cls_head_out(s + a.bc[l], a.flags);
    }
}

DeviceFlags g_cls_head_configured;

bool args_ok(const ClsHeadArgs &a) { return a.B > 0 && a.H > 0 && a.n_labels >= 1 && a.n_labels <= CLS_HEAD_MAX_LABELS && a.rows && a.bp && a.wc && a.bc && a.out; }

}  // namespace

bool cls_head_mfma_supported(int H) { return H >= 8 && H % 8 == 0 && H <= CLS_HEAD_MFMA_MAX_H; }

size_t cls_head_lds_bytes(int H) { return (size_t)CH_SB * (H + 8) * 2 + (size_t)CH_WAVES * CH_NL * 32 * sizeof(float); }

bool launch_cls_head(const ClsHeadArgs &a, hipStream_t s) {
    if (!args_ok(a) || !a.wp16 || !cls_head_mfma_supported(a.H)) return false;
    // (from H = 968 on the staged rows and the waves' sums pass the 64 KiB a kernel gets without asking: 70 144 bytes at H = 1024)
    configure_once(g_cls_head_configured, [] { (void)hipFuncSetAttribute((const void *)cls_head_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cls_head_lds_bytes(CLS_HEAD_MFMA_MAX_H)); });
    BERT_LAUNCH(cls_head_kernel, dim3((unsigned)((a.B + CH_SB - 1) / CH_SB)), dim3(CH_NT), cls_head_lds_bytes(a.H), s, a);
    return true;
}

bool launch_cls_head_f32(const ClsHeadArgs &a, hipStream_t s) {
    if (!args_ok(a) || (!a.wp32 && !a.wp16) || a.H > 8192) return false;
    const size_t lds = (size_t)2 * a.H * sizeof(float);
    if (a.wp32) BERT_LAUNCH(cls_head_f32_kernel<float>, dim3((unsigned)a.B), dim3(CH_NT), lds, s, a, a.wp32);
    else BERT_LAUNCH(cls_head_f32_kernel<half_t>, dim3((unsigned)a.B), dim3(CH_NT), lds, s, a, a.wp16);
    return true;
}

}  // namespace bert_hip
