// test_api.hip — standalone kernel entry points of bert_hip.h for op-level parity tests.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bert_hip_test.h"
#include <stdexcept>

#include "context.h"
#include "index_file.h"
#include "sparse_index_file.h"
#include "partition.h"
#include "search.h"

using namespace bert_hip;

#define CK(expr)                                                                       \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__));                \
            return -1;                                                                 \
        }                                                                              \
    } while (0)

// skinny_layer_supported judges a whole layer.  An entry that holds only some of its matrices passes stand-ins for the others:
// `like`'s type and image pointers (that they are there is all the predicate asks of them) under the shape a layer gives them.
static GemmWeight stand_in(const GemmWeight &like, int N, int K) {
    GemmWeight w = like;
    w.N = w.N_pad = N; w.K = K; w.w16p = like.w16;
    return w;
}
static bool skinny_qkv_supported(const GemmWeight &Wqkv) {
    const int H = Wqkv.K;
    return skinny_layer_supported(Wqkv, stand_in(Wqkv, H, H), stand_in(Wqkv, 4 * H, H), stand_in(Wqkv, H, 4 * H));
}

// rows [M][cols] of 16- or 32-bit words -> device rows [M_pad][cols], rows M .. M_pad - 1 filled with `pad` (the kernels compute
// whole token blocks, and in a reused workspace those rows hold whatever the call before left); src == nullptr: all rows `pad`
template <class T>
static bool upload_padded(DevBuf &d, const T *src, int M, int M_pad, int cols, T pad, std::string &err) {
    std::vector<T> h((size_t)M_pad * cols, pad);
    if (src) memcpy(h.data(), src, (size_t)M * cols * sizeof(T));
    return d.upload(h, err);
}

// bert_hip_test_set_pad: what the batch-route entries put where a call writes nothing before the first launch (0, 0: zeros, the
// state DevBuf::alloc leaves).  The engine's workspaces hold whatever an earlier pass left there.
static uint16_t g_pad16 = 0;
static uint32_t g_pad32 = 0;
// rows [M][cols] of f16 bits (src == nullptr: none) -> device rows [M_pad][cols], the rows behind them holding the 16-bit pattern
static bool upload_rows16(DevBuf &d, const uint16_t *src, int M, int M_pad, int cols, std::string &err) {
    return upload_padded(d, src, src ? M : 0, M_pad, cols, g_pad16, err);
}
// an output or intermediate buffer of n 16-bit / 32-bit words, every word the pattern
static bool alloc_pad16(DevBuf &d, size_t n, std::string &err) { return g_pad16 ? d.upload(std::vector<uint16_t>(n, g_pad16), err) : d.alloc(n * 2, err); }
static bool alloc_pad32(DevBuf &d, size_t n, std::string &err) { return g_pad32 ? d.upload(std::vector<uint32_t>(n, g_pad32), err) : d.alloc(n * 4, err); }

// the matrices and parameter vectors of a layer tail on the device, from file-layout bytes (W1, W2 also in the k order of w16p)
struct TailOperands {
    GemmWeightStore wo, w1, w2;
    DevBuf bo, g1, be1, b1, b2, g2, be2;
    // 0; -1 with a line on stderr; -2: a matrix the MFMA kernels do not take
    int build(const char *me, int H, int I, const void *Wo, const void *W1, const void *W2, int32_t wtype, const float *bo_, const float *g1_,
              const float *be1_, const float *b1_, const float *b2_, const float *g2_, const float *be2_) {
        std::string err;
        HostTensor to, t1, t2;
        to.type = wtype; to.n_dims = 2; to.ne0 = H; to.ne1 = H; to.data = (const uint8_t *)Wo; to.nbytes = wtype_row_bytes(wtype, H) * (size_t)H;
        t1.type = wtype; t1.n_dims = 2; t1.ne0 = H; t1.ne1 = I; t1.data = (const uint8_t *)W1; t1.nbytes = wtype_row_bytes(wtype, H) * (size_t)I;
        t2.type = wtype; t2.n_dims = 2; t2.ne0 = I; t2.ne1 = H; t2.data = (const uint8_t *)W2; t2.nbytes = wtype_row_bytes(wtype, I) * (size_t)H;
        PackOptions kperm;
        kperm.kperm = true;
        if (!wo.build({&to}, PackOptions(), err) || !w1.build({&t1}, kperm, err) || !w2.build({&t2}, kperm, err) ||
            !bo.upload(bo_, (size_t)H * 4, err) || !g1.upload(g1_, (size_t)H * 4, err) || !be1.upload(be1_, (size_t)H * 4, err) ||
            !b1.upload(b1_, (size_t)I * 4, err) || !b2.upload(b2_, (size_t)H * 4, err) || !g2.upload(g2_, (size_t)H * 4, err) ||
            !be2.upload(be2_, (size_t)H * 4, err)) {
            fprintf(stderr, "%s: %s\n", me, err.c_str());
            return -1;
        }
        return wo.mfma_ok && w1.mfma_ok && w2.mfma_ok ? 0 : -2;
    }
};

// bert_hip_test_attention[_bias]: W [32][n_head] expanded for P tokens (or rel as it is), none for both NULL
static int32_t test_attention(const char *me, int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head, const uint16_t *qkv,
                              int32_t impl, uint16_t *out, const float *W, int32_t P, const float *rel) {
    std::string err;
    const int T = cu_seqlens[n_sentences], H = n_head * d_head;
    int max_len = 0;
    for (int b = 0; b < n_sentences; ++b) max_len = std::max(max_len, cu_seqlens[b + 1] - cu_seqlens[b]);
    // (whole token tiles, as in the engine's workspaces, and one key tile more: the kernel pads the LAST sentence's keys to 128 in LDS,
    // not from memory, and one that loaded them would find the pattern there instead of leaving the buffer)
    const int T_pad = (T + 255) / 256 * 256 + 128;
    DevBuf dq, dcu, dout, drel;
    const bool bias = W || rel;
    if (bias && (P < 1 || max_len > P || n_head < 1)) { fprintf(stderr, "%s: a sentence of %d tokens, the table is for up to %d\n", me, max_len, P); return -1; }
    if (!upload_rows16(dq, qkv, T, T_pad, 3 * H, err) || !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) ||
        !alloc_pad16(dout, (size_t)T_pad * H, err) ||
        (bias && !(rel ? drel.upload(rel, (size_t)n_head * (2 * P - 1) * 4, err)
                       : drel.upload(rel_bias_table(W, n_head, P, impl == 0 ? std::sqrt((double)d_head) : 1.0), err)))) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    const float *dr = bias ? drel.as<float>() : nullptr;
    if (impl == 0) {
        if (!launch_attention_mfma(dq.as<half_t>(), dcu.as<int32_t>(), n_sentences, n_head, d_head, max_len, dout.as<half_t>(), nullptr, dr, P)) {
            fprintf(stderr, "%s: shape not supported by the MFMA path\n", me);
            return -2;
        }
    } else {
        launch_attention_naive(dq.as<half_t>(), dcu.as<int32_t>(), n_sentences, n_head, d_head, max_len, dout.as<half_t>(), nullptr, dr, P);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)T * H * 2, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" {

int32_t bert_hip_test_gemm(int32_t M, int32_t N, int32_t K, const uint16_t *A, const void *W, int32_t wtype,
                           const float *bias, const uint16_t *resid, int32_t epilogue, int32_t impl, uint16_t *C) {
    std::string err;
    HostTensor t;
    t.type = wtype; t.n_dims = 2; t.ne0 = K; t.ne1 = N; t.data = (const uint8_t *)W;
    t.nbytes = wtype_row_bytes(wtype, K) * (size_t)N;
    GemmWeightStore ws;
    if (!ws.build({&t}, PackOptions{impl == 1}, err)) { fprintf(stderr, "bert_hip_test_gemm: %s\n", err.c_str()); return -1; }
    if (impl != 1 && !ws.mfma_ok) { fprintf(stderr, "bert_hip_test_gemm: shape not supported by the MFMA path\n"); return -2; }
    const int M_pad = impl == 3 ? (M + 255) / 256 * 256 : (M + GEMM_BM - 1) / GEMM_BM * GEMM_BM;
    DevBuf dA, dB, dR, dC;
    if (!upload_rows16(dA, A, M, M_pad, K, err) || !alloc_pad16(dC, (size_t)M_pad * N, err) || !dB.upload(bias, (size_t)N * 4, err) ||
        (resid && !upload_rows16(dR, resid, M, M_pad, N, err))) {
        fprintf(stderr, "bert_hip_test_gemm: %s\n", err.c_str());
        return -1;
    }
    if (impl == 3) {
        if (!gemm256_supported(ws.w, M_pad)) return -2;
        if (!launch_gemm256(ws.w, dA.as<half_t>(), dB.as<float>(), dR.as<half_t>(), dC.as<half_t>(), M_pad, epilogue, nullptr)) return -3;
    } else if (impl == 0) launch_gemm_mfma(ws.w, dA.as<half_t>(), dB.as<float>(), dR.as<half_t>(), dC.as<half_t>(), M_pad, epilogue, nullptr);
    else launch_gemm_naive(ws.w, dA.as<half_t>(), dB.as<float>(), dR.as<half_t>(), dC.as<half_t>(), M, epilogue, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(C, dC.p, (size_t)M * N * 2, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_gemm_lnfold(int32_t M, int32_t K1, int32_t H, int32_t N2, const uint16_t *A1, const uint16_t *W1, const float *b1,
                                  const uint16_t *r, const float *rg, const float *rb, const uint16_t *W2, const float *b2, const float *g,
                                  const float *be, int32_t epi2, uint16_t *u_out, uint16_t *out2, float *rows_out) {
    std::string err;
    auto tensor = [](const uint16_t *w, int n, int k) {
        HostTensor t;
        t.type = W_F16; t.n_dims = 2; t.ne0 = k; t.ne1 = n; t.data = (const uint8_t *)w; t.nbytes = (size_t)n * k * 2;
        return t;
    };
    const HostTensor t1 = tensor(W1, H, K1), t2 = tensor(W2, N2, H);
    GemmWeightStore w1, w2;
    DevBuf waug, gb;
    if (!w1.build({&t1}, PackOptions(), err) || !w2.build_ln_fold({&t2}, g, be, b2, waug, err)) { fprintf(stderr, "bert_hip_test_gemm_lnfold: %s\n", err.c_str()); return -1; }
    const int M_pad = (M + 255) / 256 * 256, P = 2 * H / 256;
    if (!gemm256_supported(w1.w, M_pad) || !gemm256_supported(w2.w, M_pad) || H % 256) return -2;
    DevBuf dA, dB1, dR, dU, dOut, dStats, dRows, dRowsRes;
    if (!upload_rows16(dA, A1, M, M_pad, K1, err) || !dB1.upload(b1, (size_t)H * 4, err) || !upload_rows16(dR, r, M, M_pad, H, err) ||
        !alloc_pad16(dU, (size_t)M_pad * H, err) || !alloc_pad16(dOut, (size_t)M_pad * N2, err) || !alloc_pad32(dStats, (size_t)M_pad * P * 2, err) ||
        !alloc_pad32(dRows, (size_t)M_pad * 4, err) || (!rg && !alloc_pad32(dRowsRes, (size_t)M_pad * 4, err))) return -1;
    GemmLnFold ln;
    ln.flags = GemmLnFold::STATS; ln.stats = dStats.as<float2>();
    if (rg) {
        // the residual's own row statistics (what the mat-mul that produced r would have left behind), and the packed (gamma, beta + bias)
        float pad_f;
        memcpy(&pad_f, &g_pad32, 4);
        std::vector<float> rows((size_t)M_pad * 4, pad_f);
        for (int t = 0; t < M; ++t) {
            double s1 = 0, s2 = 0;
            for (int f = 0; f < H; ++f) { _Float16 h; memcpy(&h, &r[(size_t)t * H + f], 2); s1 += (double)(float)h; s2 += (double)(float)h * (double)(float)h; }
            const double mean = s1 / H, var = std::max(s2 / H - mean * mean, 0.0) + 1e-5, sd = std::sqrt(var);
            rows[4 * (size_t)t] = (float)(1.0 / sd); rows[4 * (size_t)t + 1] = (float)(-mean / sd); rows[4 * (size_t)t + 2] = (float)-mean; rows[4 * (size_t)t + 3] = (float)sd;
        }
        if (!dRowsRes.upload(rows, err)) return -1;
        std::vector<uint32_t> v((size_t)H);
        for (int f = 0; f < H; ++f) {
            const _Float16 gg = (_Float16)rg[f], bb = (_Float16)(rb[f] + b1[f]);
            uint16_t gu, bu; memcpy(&gu, &gg, 2); memcpy(&bu, &bb, 2);
            v[(size_t)f] = (uint32_t)gu | ((uint32_t)bu << 16);
        }
        if (!gb.upload(v.data(), v.size() * 4, err)) return -1;
        ln.flags |= GemmLnFold::RES; ln.rows_res = dRowsRes.as<float4>(); ln.gb = gb.as<unsigned>();
    }
    bool ran = launch_gemm256(w1.w, dA.as<half_t>(), dB1.as<float>(), dR.as<half_t>(), dU.as<half_t>(), M_pad, EPI_BIAS_RESID, nullptr, &ln);
    if (ran) launch_ln_rows_finalize(dStats.as<float2>(), P, M_pad, H, dRows.as<float4>(), nullptr);
    GemmLnFold in;
    in.flags = GemmLnFold::IN; in.rows_in = dRows.as<float4>(); in.waug = waug.as<half_t>();
    ran = ran && launch_gemm256(w2.w, dU.as<half_t>(), nullptr, nullptr, dOut.as<half_t>(), M_pad, epi2, nullptr, &in);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (!ran) { fprintf(stderr, "bert_hip_test_gemm_lnfold: launch_gemm256 has no kernel for this LayerNorm-folding form (epilogue %d)\n", epi2); return -3; }
    CK(hipMemcpy(u_out, dU.p, (size_t)M * H * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(out2, dOut.p, (size_t)M * N2 * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rows_out, dRows.p, (size_t)M * 16, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head,
                                const uint16_t *qkv, int32_t impl, uint16_t *out) {
    return test_attention("bert_hip_test_attention", n_sentences, cu_seqlens, n_head, d_head, qkv, impl, out, nullptr, 0, nullptr);
}

int32_t bert_hip_test_attention_bias(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head, const uint16_t *qkv,
                                     int32_t impl, uint16_t *out, const float *W, int32_t P, const float *rel) {
    if (!W && !rel) { fprintf(stderr, "bert_hip_test_attention_bias: W or rel required\n"); return -1; }
    return test_attention("bert_hip_test_attention_bias", n_sentences, cu_seqlens, n_head, d_head, qkv, impl, out, W, P, rel);
}

int32_t bert_hip_test_rel_bias_table(const float *W, int32_t n_head, int32_t P, float *out) {
    if (!W || !out || n_head < 1 || P < 1) return -1;
    const std::vector<float> rel = rel_bias_table(W, n_head, P, 1.0);
    memcpy(out, rel.data(), rel.size() * 4);
    return 0;
}

int32_t bert_hip_test_qkv_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head,
                                    const uint16_t *x, const void *Wqkv, int32_t wtype, const float *bias, int32_t fused,
                                    uint16_t *out) {
    std::string err;
    const int T = cu_seqlens[n_sentences], H = n_head * d_head;
    const int T_pad = (T + GEMM_BM - 1) / GEMM_BM * GEMM_BM;
    int max_len = 0;
    for (int b = 0; b < n_sentences; ++b) max_len = std::max(max_len, cu_seqlens[b + 1] - cu_seqlens[b]);
    HostTensor t;
    t.type = wtype; t.n_dims = 2; t.ne0 = H; t.ne1 = 3 * H; t.data = (const uint8_t *)Wqkv;
    t.nbytes = wtype_row_bytes(wtype, H) * (size_t)3 * H;
    GemmWeightStore ws;
    if (!ws.build({&t}, PackOptions(), err)) { fprintf(stderr, "bert_hip_test_qkv_attention: %s\n", err.c_str()); return -1; }
    if (!ws.mfma_ok) return -2;
    DevBuf dx, dqkv, dcu, db, dout;
    // (x and qkv: one window more than T_pad rows — the window kernel's empty slots must not read their own rows nor the attention
    // kernel the keys behind the last sentence, and a kernel that did would find the pattern there instead of leaving the buffer)
    if (!upload_rows16(dx, x, T, T_pad + 128, H, err) || !alloc_pad16(dqkv, (size_t)(T_pad + 128) * 3 * H, err) ||
        !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) || !db.upload(bias, (size_t)3 * H * 4, err) ||
        !alloc_pad16(dout, (size_t)T_pad * H, err)) {
        fprintf(stderr, "bert_hip_test_qkv_attention: %s\n", err.c_str());
        return -1;
    }
    if (fused >= 2 && fused <= 4) {
        // second-generation kernel: 2 = next-fit windows of whole sentences, 3 = the uniform placement rule
        if (!qkv_attention2_supported(ws.w, n_head, d_head, max_len)) return -2;
        std::vector<int2> win;
        DevBuf dwin;
        DevBuf dcount;
        int n_win = 0;
        if (fused == 2) {
            Engine::build_windows(cu_seqlens, n_sentences, win, window_slots());
            if (!dwin.upload(win.data(), win.size() * sizeof(int2), err)) return -1;
            n_win = (int)win.size();
        } else if (fused == 4) {
            // the same windows built on the device; the grid is the launcher's upper bound
            if (!dwin.alloc((size_t)n_sentences * sizeof(int2), err) || !dcount.alloc(sizeof(int), err)) return -1;
            launch_build_windows(dcu.as<int32_t>(), n_sentences, dwin.as<int2>(), dcount.as<int>(), window_slots(), nullptr);
            n_win = qkv_attention2_max_windows(n_sentences, T, window_slots());
        }
        launch_qkv_attention2(ws.w, dx.as<half_t>(), db.as<float>(), dcu.as<int32_t>(), n_sentences,
                              fused == 3 ? nullptr : dwin.as<int2>(), n_win, fused == 4 ? dcount.as<int>() : nullptr, max_len, n_head,
                              window_slots(), dout.as<half_t>(), nullptr);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
    } else if (fused == 5) {
        // the first half of a latency-route layer as Engine::forward_latency chains it (first layer: x comes as f16 rows)
        if (!skinny_qkv_supported(ws.w)) return -2;
        launch_skinny_gemm(0, ws.w, dx.as<half_t>(), nullptr, nullptr, nullptr, dx.as<half_t>(), db.as<float>(), nullptr, dqkv.as<half_t>(), nullptr,
                           (T + 31) / 32, nullptr);
        if (!launch_attention_mfma(dqkv.as<half_t>(), dcu.as<int32_t>(), n_sentences, n_head, d_head, max_len, dout.as<half_t>(), nullptr))
            return -2;
    } else {
        launch_gemm_mfma(ws.w, dx.as<half_t>(), db.as<float>(), nullptr, dqkv.as<half_t>(), T_pad, EPI_BIAS, nullptr);
        if (!launch_attention_mfma(dqkv.as<half_t>(), dcu.as<int32_t>(), n_sentences, n_head, d_head, max_len, dout.as<half_t>(), nullptr))
            return -2;
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)T * H * 2, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_layer_tail(int32_t M, int32_t H, int32_t I, const uint16_t *ctx, const uint16_t *x, const void *Wo,
                                 const void *W1, const void *W2, int32_t wtype, const float *bo, const float *g1,
                                 const float *be1, const float *b1, const float *b2, const float *g2, const float *be2,
                                 int32_t impl, uint16_t *out) {
    std::string err;
    TailOperands w;
    if (const int r = w.build("bert_hip_test_layer_tail", H, I, Wo, W1, W2, wtype, bo, g1, be1, b1, b2, g2, be2)) return r;
    const int M_pad = (M + GEMM_BM - 1) / GEMM_BM * GEMM_BM;
    DevBuf dc, dx, dy, dout;
    if (!upload_rows16(dc, ctx, M, M_pad, H, err) || !upload_rows16(dx, x, M, M_pad, H, err) || !alloc_pad16(dy, (size_t)M_pad * H, err) ||
        !alloc_pad16(dout, (size_t)M_pad * H, err)) {
        fprintf(stderr, "bert_hip_test_layer_tail: %s\n", err.c_str());
        return -1;
    }
    if (impl == 1) {
        if (!layer_tail_supported(w.wo.w, w.w1.w, w.w2.w)) return -2;
        launch_layer_tail(w.wo.w, w.w1.w, w.w2.w, dc.as<half_t>(), dx.as<half_t>(), w.bo.as<float>(), w.g1.as<float>(), w.be1.as<float>(),
                          w.b1.as<float>(), w.b2.as<float>(), w.g2.as<float>(), w.be2.as<float>(), dout.as<half_t>(), M_pad, nullptr);
    } else {
        // three GEMM kernels + two LayerNorm kernels
        DevBuf dff;
        if (!alloc_pad16(dff, (size_t)M_pad * I, err)) return -1;
        launch_gemm_mfma(w.wo.w, dc.as<half_t>(), w.bo.as<float>(), dx.as<half_t>(), dy.as<half_t>(), M_pad, EPI_BIAS_RESID, nullptr);
        launch_layernorm(dy.as<half_t>(), w.g1.as<float>(), w.be1.as<float>(), M_pad, H, nullptr);
        launch_gemm_mfma(w.w1.w, dy.as<half_t>(), w.b1.as<float>(), nullptr, dff.as<half_t>(), M_pad, EPI_BIAS_GELU, nullptr);
        launch_gemm_mfma(w.w2.w, dff.as<half_t>(), w.b2.as<float>(), dy.as<half_t>(), dout.as<half_t>(), M_pad, EPI_BIAS_RESID, nullptr);
        launch_layernorm(dout.as<half_t>(), w.g2.as<float>(), w.be2.as<float>(), M_pad, H, nullptr);
        CK(hipDeviceSynchronize());
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)M * H * 2, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_skinny_tail(int32_t M, int32_t H, int32_t I, const uint16_t *ctx, const uint16_t *x, const void *Wo, const void *W1,
                                  const void *W2, int32_t wtype, const float *bo, const float *g1, const float *be1, const float *b1,
                                  const float *b2, const float *g2, const float *be2, uint32_t pad, uint16_t *out, float *v_proj,
                                  uint16_t *y, uint16_t *ff, float *v_down) {
    std::string err;
    TailOperands w;
    if (const int r = w.build("bert_hip_test_skinny_tail", H, I, Wo, W1, W2, wtype, bo, g1, be1, b1, b2, g2, be2)) return r;
    if (!skinny_layer_supported(stand_in(w.wo.w, 3 * H, H), w.wo.w, w.w1.w, w.w2.w)) return -2;
    const int M_pad = (M + GEMM_BM - 1) / GEMM_BM * GEMM_BM, tb = (M + 31) / 32;
    DevBuf dc, dx, dy, dff, dv;
    if (!upload_padded(dc, ctx, M, M_pad, H, (uint16_t)pad, err) || !upload_padded(dx, x, M, M_pad, H, (uint16_t)pad, err) ||
        !dy.alloc((size_t)M_pad * H * 2, err) || !dff.alloc((size_t)M_pad * I * 2, err) || !dv.alloc((size_t)M_pad * H * 4, err)) {
        fprintf(stderr, "bert_hip_test_skinny_tail: %s\n", err.c_str());
        return -1;
    }
    half_t *xd = dx.as<half_t>(), *yd = dy.as<half_t>(), *ffd = dff.as<half_t>();
    float *v32 = dv.as<float>();
    // (Engine::forward_latency's launches and arguments; the f32 rows of both residual mat-muls share one buffer there)
    launch_skinny_gemm(1, w.wo.w, dc.as<half_t>(), nullptr, nullptr, nullptr, nullptr, w.bo.as<float>(), xd, nullptr, v32, tb, nullptr);
    if (v_proj) {
        CK(hipGetLastError());
        CK(hipMemcpy(v_proj, v32, (size_t)M * H * 4, hipMemcpyDeviceToHost));
    }
    launch_skinny_gemm(2, w.w1.w, nullptr, v32, w.g1.as<float>(), w.be1.as<float>(), yd, w.b1.as<float>(), nullptr, ffd, nullptr, tb, nullptr);
    launch_skinny_gemm(3, w.w2.w, ffd, nullptr, nullptr, nullptr, nullptr, w.b2.as<float>(), yd, nullptr, v32, tb, nullptr);
    if (v_down) {
        CK(hipGetLastError());
        CK(hipMemcpy(v_down, v32, (size_t)M * H * 4, hipMemcpyDeviceToHost));
    }
    launch_skinny_layernorm(v32, w.g2.as<float>(), w.be2.as<float>(), xd, tb, H, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, xd, (size_t)M * H * 2, hipMemcpyDeviceToHost));
    if (y) CK(hipMemcpy(y, yd, (size_t)M * H * 2, hipMemcpyDeviceToHost));
    if (ff) CK(hipMemcpy(ff, ffd, (size_t)M * I * 2, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_skinny_qkv(int32_t M, int32_t H, const uint16_t *x, const float *V, const float *gamma, const float *beta,
                                 const void *Wqkv, int32_t wtype, const float *bias, uint32_t pad, uint16_t *qkv, uint16_t *ln_out) {
    std::string err;
    if ((V == nullptr) == (x == nullptr) || (V && (!gamma || !beta || !ln_out))) return -1;
    HostTensor t;
    t.type = wtype; t.n_dims = 2; t.ne0 = H; t.ne1 = 3 * H; t.data = (const uint8_t *)Wqkv;
    t.nbytes = wtype_row_bytes(wtype, H) * (size_t)3 * H;
    GemmWeightStore ws;
    if (!ws.build({&t}, PackOptions(), err)) { fprintf(stderr, "bert_hip_test_skinny_qkv: %s\n", err.c_str()); return -1; }
    if (!ws.mfma_ok || !skinny_qkv_supported(ws.w)) return -2;
    const int M_pad = (M + GEMM_BM - 1) / GEMM_BM * GEMM_BM, tb = (M + 31) / 32;
    DevBuf dx, dv, dg, dbe, db, dqkv;
    // (the LayerNorm-fused form writes x: the rows are its ln_out, as in the engine)
    if (!upload_padded(dx, x, M, M_pad, H, (uint16_t)(V ? 0 : pad), err) || !dqkv.alloc((size_t)M_pad * 3 * H * 2, err) ||
        !db.upload(bias, (size_t)3 * H * 4, err) ||
        (V && (!upload_padded(dv, (const uint32_t *)V, M, M_pad, H, pad, err) || !dg.upload(gamma, (size_t)H * 4, err) ||
               !dbe.upload(beta, (size_t)H * 4, err)))) {
        fprintf(stderr, "bert_hip_test_skinny_qkv: %s\n", err.c_str());
        return -1;
    }
    half_t *xd = dx.as<half_t>();
    launch_skinny_gemm(0, ws.w, xd, V ? dv.as<float>() : nullptr, V ? dg.as<float>() : nullptr, V ? dbe.as<float>() : nullptr, xd,
                       db.as<float>(), nullptr, dqkv.as<half_t>(), nullptr, tb, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(qkv, dqkv.p, (size_t)M * 3 * H * 2, hipMemcpyDeviceToHost));
    if (V) CK(hipMemcpy(ln_out, xd, (size_t)M * H * 2, hipMemcpyDeviceToHost));
    return 0;
}


// ---- the f16 row kernels of misc_kernels.hip, launched as Engine::forward_layers launches them ----
// Token-row buffers have the engine's workspace shape, whole tiles of 256 rows, the rows behind T holding the 16-bit pattern.
static int rows_pad256(int T) { return (std::max(T, 1) + 255) / 256 * 256; }
// rows [M][cols] of the device buffer to the host; -4 if a word of rows M .. M_pad - 1 no longer holds the pattern (a store behind the
// last token: in the engine, into another pass's rows)
static int download_rows16(const char *me, uint16_t *dst, const DevBuf &d, int M, int M_pad, int cols) {
    std::vector<uint16_t> h((size_t)M_pad * cols);
    CK(hipMemcpy(h.data(), d.p, h.size() * 2, hipMemcpyDeviceToHost));
    memcpy(dst, h.data(), (size_t)M * cols * 2);
    for (size_t i = (size_t)M * cols; i < h.size(); ++i)
        if (h[i] != g_pad16) { fprintf(stderr, "%s: row %zu behind the last token was written\n", me, i / cols); return -4; }
    return 0;
}

int32_t bert_hip_test_embed_ln(int32_t table_type, int32_t H, int32_t n_vocab, int32_t n_pos, const void *word, const void *type,
                               const void *pos, const float *gamma, const float *beta, const bert_vocab_id *tokens,
                               const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len, uint16_t *out) {
    std::string err;
    if (H <= 0 || n_vocab <= 0 || n_sentences <= 0 || max_len < 0 || max_len > n_pos) return -1;       // (max_len <= n_max_tokens: bert_hip_eval_packed_device's check)
    const int T = cu_seqlens[n_sentences], T_pad = rows_pad256(T);
    if (max_len == 0)
        for (int b = 0; b < n_sentences; ++b) max_len = std::max(max_len, cu_seqlens[b + 1] - cu_seqlens[b]);
    if (max_len > n_pos) return -1;
    const size_t rb = wtype_row_bytes(table_type, H);
    DevBuf dw, dt, dp, dg, db, dtok, dcu, dout;
    if (!dw.upload(word, rb * n_vocab, err) || !dt.upload(type, rb * 2, err) || !dp.upload(pos, rb * n_pos, err) ||
        !dg.upload(gamma, (size_t)H * 4, err) || !db.upload(beta, (size_t)H * 4, err) || !dtok.upload(tokens, (size_t)T * 4, err) ||
        !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) || !alloc_pad16(dout, (size_t)T_pad * H, err)) {
        fprintf(stderr, "bert_hip_test_embed_ln: %s\n", err.c_str());
        return -1;
    }
    launch_embed_ln(dw.p, dt.p, dp.p, table_type, dg.as<float>(), db.as<float>(), dtok.as<int32_t>(), dcu.as<int32_t>(), n_sentences,
                    T, H, n_vocab, max_len, dout.as<half_t>(), nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows16("bert_hip_test_embed_ln", out, dout, T, T_pad, H);
}

// the lane-order form (launch_embed_ln_lanes): `out` gets the [T][H] halves as the kernel stored them; -2, and no launch, for a shape
// the launcher declines
int32_t bert_hip_test_embed_ln_lanes(int32_t table_type, int32_t H, int32_t n_vocab, int32_t n_pos, const void *word, const void *type,
                                     const void *pos, const float *gamma, const float *beta, const bert_vocab_id *tokens,
                                     const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len, uint16_t *out) {
    std::string err;
    if (H <= 0 || n_vocab <= 0 || n_sentences <= 0 || max_len < 0 || max_len > n_pos) return -1;
    const int T = cu_seqlens[n_sentences], T_pad = rows_pad256(T);
    if (max_len == 0)
        for (int b = 0; b < n_sentences; ++b) max_len = std::max(max_len, cu_seqlens[b + 1] - cu_seqlens[b]);
    if (max_len > n_pos) return -1;
    if (!embed_ln_lanes_supported(table_type, H, T, max_len)) return -2;
    const size_t rb = wtype_row_bytes(table_type, H);
    DevBuf dw, dt, dp, dg, db, dtok, dcu, dout;
    if (!dw.upload(word, rb * n_vocab, err) || !dt.upload(type, rb * 2, err) || !dp.upload(pos, rb * n_pos, err) ||
        !dg.upload(gamma, (size_t)H * 4, err) || !db.upload(beta, (size_t)H * 4, err) || !dtok.upload(tokens, (size_t)T * 4, err) ||
        !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) || !alloc_pad16(dout, (size_t)T_pad * H, err)) {
        fprintf(stderr, "bert_hip_test_embed_ln_lanes: %s\n", err.c_str());
        return -1;
    }
    if (!launch_embed_ln_lanes(dw.p, dt.p, dp.p, table_type, dg.as<float>(), db.as<float>(), dtok.as<int32_t>(), dcu.as<int32_t>(), n_sentences,
                               T, H, n_vocab, max_len, dout.as<half_t>(), nullptr)) return -2;
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows16("bert_hip_test_embed_ln_lanes", out, dout, T, T_pad, H);
}

int32_t bert_hip_test_layernorm(int32_t T, int32_t H, const uint16_t *x, const float *gamma, const float *beta, uint16_t *out) {
    std::string err;
    if (T <= 0 || H <= 0 || H % 2 || H > 4096) return -1;       // (the widths a model file may have: checked at load)
    const int T_pad = rows_pad256(T);
    DevBuf dx, dg, db;
    if (!upload_rows16(dx, x, T, T_pad, H, err) || !dg.upload(gamma, (size_t)H * 4, err) || !db.upload(beta, (size_t)H * 4, err)) {
        fprintf(stderr, "bert_hip_test_layernorm: %s\n", err.c_str());
        return -1;
    }
    launch_layernorm(dx.as<half_t>(), dg.as<float>(), db.as<float>(), T, H, nullptr);       // (in place, as in the engine)
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows16("bert_hip_test_layernorm", out, dx, T, T_pad, H);
}

// x [T][H] f16 bits -> the sentences' rows by the rule pool_mode names (kernels.h POOL_*), and the status word
static int32_t test_pool(const char *me, int32_t H, const uint16_t *x, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len,
                         int pool_mode, float *out, int32_t *status) {
    std::string err;
    const int T = cu_seqlens[n_sentences];
    DevBuf dx, dcu, dout, dst;
    if (!dx.upload(x, (size_t)T * H * 2, err) || !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) ||
        !dout.alloc((size_t)n_sentences * H * 4, err) || !dst.alloc(16, err)) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    launch_pool_normalize(dx.as<half_t>(), dcu.as<int32_t>(), n_sentences, H, max_len, dst.as<int>(), dout.as<float>(), pool_mode, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)n_sentences * H * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(status, dst.p, 4, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_pool_normalize(int32_t H, const uint16_t *x, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len,
                                     float *out, int32_t *status) {
    return test_pool("bert_hip_test_pool_normalize", H, x, cu_seqlens, n_sentences, max_len, 0, out, status);
}

int32_t bert_hip_test_pool(int32_t H, const uint16_t *x, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len, int32_t pooling,
                           int32_t normalize, float *out, int32_t *status) {
    return test_pool("bert_hip_test_pool", H, x, cu_seqlens, n_sentences, max_len, (pooling ? POOL_CLS : 0) | (normalize ? 0 : POOL_RAW), out,
                     status);
}

int32_t bert_hip_test_group_pool(const float *rows, int32_t n_rows, const int32_t *weights, const int32_t *group_cu, int32_t n_groups, int32_t H,
                                 int32_t raw, float *out, int32_t *status) {
    const char *me = "bert_hip_test_group_pool";
    if (!rows || !group_cu || !out || n_rows < 1 || n_groups < 1 || H < 1) return -1;
    std::string err;
    // the weights as the engine has them: prefix sums of the sentences' token counts
    std::vector<int32_t> cu((size_t)n_rows + 1, 0);
    if (weights)
        for (int32_t s = 0; s < n_rows; ++s) cu[s + 1] = cu[s] + weights[s];
    DevBuf drows, dcu, dg, dout, dst;
    if (!drows.upload(rows, (size_t)n_rows * H * 4, err) || !dcu.upload(cu, err) || !dg.upload(group_cu, (size_t)(n_groups + 1) * 4, err) ||
        !dout.upload(out, (size_t)n_groups * H * 4, err) || !dst.alloc(16, err)) {           // (out: what the caller put there stays where the kernel does not write)
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    launch_group_pool(drows.as<float>(), weights ? dcu.as<int32_t>() : nullptr, dg.as<int32_t>(), n_rows, n_groups, H, raw != 0, dst.as<int>(), dout.as<float>(), nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)n_groups * H * 4, hipMemcpyDeviceToHost));
    if (status) CK(hipMemcpy(status, dst.p, 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- the f32 route's kernels (f32_route.hip), launched as Engine::forward_f32 launches them ----
// The engine's workspaces hold whole 256-token tiles: token-row buffers get T_pad rows, the rows behind T holding the 32-bit pattern.
static int f32_rows_pad(int T) { return (std::max(T, 1) + 255) / 256 * 256; }
static bool upload_rows32(DevBuf &d, const float *src, int M, int M_pad, int cols, std::string &err) {
    return upload_padded(d, (const uint32_t *)src, src ? M : 0, M_pad, cols, g_pad32, err);
}
// rows [M][cols] of the device buffer to the host; -4 if a word of rows M .. M_pad - 1 no longer holds the pattern (a store behind the
// last token: in the engine, into another pass's rows)
static int download_rows32(const char *me, float *dst, const DevBuf &d, int M, int M_pad, int cols) {
    std::vector<uint32_t> h((size_t)M_pad * cols);
    CK(hipMemcpy(h.data(), d.p, h.size() * 4, hipMemcpyDeviceToHost));
    memcpy(dst, h.data(), (size_t)M * cols * 4);
    for (size_t i = (size_t)M * cols; i < h.size(); ++i)
        if (h[i] != g_pad32) { fprintf(stderr, "%s: row %zu behind the last token was written\n", me, i / cols); return -4; }
    return 0;
}

int32_t bert_hip_test_f32_gemm(int32_t M, int32_t N, int32_t K, const float *A, const float *W, const float *bias, const float *resid,
                               int32_t epilogue, float *C) {
    std::string err;
    if (M <= 0 || N <= 0 || K <= 0 || epilogue < 0 || epilogue > 2 || (epilogue == EPI_BIAS_RESID) != (resid != nullptr)) return -1;
    const int M_pad = f32_rows_pad(M);
    DevBuf dA, dW, dB, dR, dC;
    if (!upload_rows32(dA, A, M, M_pad, K, err) || !dW.upload(W, (size_t)N * K * 4, err) || !dB.upload(bias, (size_t)N * 4, err) ||
        (resid && !upload_rows32(dR, resid, M, M_pad, N, err)) || !alloc_pad32(dC, (size_t)M_pad * N, err)) {
        fprintf(stderr, "bert_hip_test_f32_gemm: %s\n", err.c_str());
        return -1;
    }
    launch_f32_gemm(dA.as<float>(), dW.as<float>(), dB.as<float>(), dR.as<float>(), dC.as<float>(), M, N, K, epilogue, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows32("bert_hip_test_f32_gemm", C, dC, M, M_pad, N);
}

// bert_hip_test_f32_attention[_bias]: W [32][n_head] expanded for P tokens, NULL: none
static int32_t test_f32_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head, int32_t max_len,
                                  const float *qkv, float *out, const float *W, int32_t P);
int32_t bert_hip_test_f32_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head, int32_t max_len,
                                    const float *qkv, float *out) {
    return test_f32_attention(n_sentences, cu_seqlens, n_head, d_head, max_len, qkv, out, nullptr, 0);
}
int32_t bert_hip_test_f32_attention_bias(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head, int32_t max_len,
                                         const float *qkv, float *out, const float *W, int32_t P) {
    if (!W || P < 1 || max_len > P) { fprintf(stderr, "bert_hip_test_f32_attention_bias: W and P >= max_len required\n"); return -1; }
    return test_f32_attention(n_sentences, cu_seqlens, n_head, d_head, max_len, qkv, out, W, P);
}
static int32_t test_f32_attention(int32_t n_sentences, const int32_t *cu_seqlens, int32_t n_head, int32_t d_head, int32_t max_len,
                                  const float *qkv, float *out, const float *W, int32_t P) {
    std::string err;
    if (n_sentences <= 0 || n_head <= 0 || d_head <= 0) return -1;
    const int T = cu_seqlens[n_sentences], H = n_head * d_head, T_pad = f32_rows_pad(T);
    DevBuf dq, dcu, dout, drel;
    if (!upload_rows32(dq, qkv, T, T_pad, 3 * H, err) || !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) ||
        !alloc_pad32(dout, (size_t)T_pad * H, err) || (W && !drel.upload(rel_bias_table(W, n_head, P, 1.0), err))) {
        fprintf(stderr, "bert_hip_test_f32_attention: %s\n", err.c_str());
        return -1;
    }
    if (!launch_f32_attention(dq.as<float>(), dcu.as<int32_t>(), n_sentences, n_head, d_head, max_len, dout.as<float>(), nullptr, W ? drel.as<float>() : nullptr, P)) {
        fprintf(stderr, "bert_hip_test_f32_attention: max_len = %d needs %zu bytes of LDS a workgroup, the device's limit is %zu\n", max_len,
                f32_attention_lds_bytes(max_len), f32_attention_lds_limit());
        return -2;
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows32("bert_hip_test_f32_attention", out, dout, T, T_pad, H);
}

int32_t bert_hip_test_f32_layernorm(int32_t T, int32_t H, const float *x, const float *gamma, const float *beta, float *out) {
    std::string err;
    if (T <= 0 || H <= 0) return -1;
    const int T_pad = f32_rows_pad(T);
    DevBuf dx, dg, db;
    if (!upload_rows32(dx, x, T, T_pad, H, err) || !dg.upload(gamma, (size_t)H * 4, err) || !db.upload(beta, (size_t)H * 4, err)) {
        fprintf(stderr, "bert_hip_test_f32_layernorm: %s\n", err.c_str());
        return -1;
    }
    launch_f32_layernorm(dx.as<float>(), dg.as<float>(), db.as<float>(), T, H, nullptr);       // (in place, as in the engine)
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows32("bert_hip_test_f32_layernorm", out, dx, T, T_pad, H);
}

int32_t bert_hip_test_f32_embed_ln(int32_t H, int32_t n_vocab, int32_t n_pos, const float *word, const float *type, const float *pos,
                                   const float *gamma, const float *beta, const bert_vocab_id *tokens, const int32_t *cu_seqlens,
                                   int32_t n_sentences, int32_t max_len, float *out) {
    std::string err;
    if (H <= 0 || n_vocab <= 0 || n_sentences <= 0 || max_len <= 0 || max_len > n_pos) return -1;     // (max_len <= n_max_tokens: bert_hip_eval_packed_device's check)
    const int T = cu_seqlens[n_sentences], T_pad = f32_rows_pad(T);
    DevBuf dw, dt, dp, dg, db, dtok, dcu, dout;
    if (!dw.upload(word, (size_t)n_vocab * H * 4, err) || !dt.upload(type, (size_t)2 * H * 4, err) || !dp.upload(pos, (size_t)n_pos * H * 4, err) ||
        !dg.upload(gamma, (size_t)H * 4, err) || !db.upload(beta, (size_t)H * 4, err) || !dtok.upload(tokens, (size_t)T * 4, err) ||
        !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) || !alloc_pad32(dout, (size_t)T_pad * H, err)) {
        fprintf(stderr, "bert_hip_test_f32_embed_ln: %s\n", err.c_str());
        return -1;
    }
    launch_f32_embed_ln(dw.as<float>(), dt.as<float>(), dp.as<float>(), dg.as<float>(), db.as<float>(), dtok.as<int32_t>(), dcu.as<int32_t>(),
                        n_sentences, T, H, n_vocab, max_len, dout.as<float>(), nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return download_rows32("bert_hip_test_f32_embed_ln", out, dout, T, T_pad, H);
}

int32_t bert_hip_test_f32_pool(int32_t H, const float *x, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len, int32_t pooling,
                               int32_t normalize, float *out, int32_t *status) {
    std::string err;
    if (H <= 0 || n_sentences <= 0) return -1;
    const int T = cu_seqlens[n_sentences], T_pad = f32_rows_pad(T);
    DevBuf dx, dcu, dout, dst;
    if (!upload_rows32(dx, x, T, T_pad, H, err) || !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) ||
        !alloc_pad32(dout, (size_t)n_sentences * H, err) || !dst.alloc(16, err)) {
        fprintf(stderr, "bert_hip_test_f32_pool: %s\n", err.c_str());
        return -1;
    }
    launch_f32_pool_normalize(dx.as<float>(), dcu.as<int32_t>(), n_sentences, H, max_len, dst.as<int>(), dout.as<float>(),
                              (pooling ? POOL_CLS : 0) | (normalize ? 0 : POOL_RAW), nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)n_sentences * H * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(status, dst.p, 4, hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_model_digest(const char *fname, int32_t *legacy_q4, uint64_t *digest) {
    ModelFile mf;
    std::string err;
    if (!mf.load(fname, false, err)) { fprintf(stderr, "bert_hip_test_model_digest: %s\n", err.c_str()); return -1; }
    uint64_t h = 1469598103934665603ull;                       // FNV-1a over name, type and bytes (current layout) of every tensor
    auto mix = [&](const void *p, size_t n) { for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t *)p)[i]; h *= 1099511628211ull; } };
    for (const auto &kv : mf.tensors) {
        mix(kv.first.data(), kv.first.size());
        mix(&kv.second.type, 4);
        mix(kv.second.data, kv.second.nbytes);
    }
    *legacy_q4 = mf.legacy_q4 ? 1 : 0;
    *digest = h;
    return (int32_t)mf.tensors.size();
}

int32_t bert_hip_test_pack_weight(const void *W, int32_t wtype, int32_t N, int32_t K, int32_t form, const float *gamma, const float *beta,
                                  const float *bias, void *out, int64_t out_cap) {
    const bool stack3 = (form & BERT_HIP_TEST_PACK_STACK3) != 0;
    form &= ~BERT_HIP_TEST_PACK_STACK3;
    const bool q4 = wtype == W_Q4_0 || wtype == W_Q4_1;
    if (!out || N <= 0 || wtype < W_F32 || wtype > W_Q4_1 || (stack3 && N % 3 != 0)) return -1;
    if (form != 6 && (!W || K <= 0 || (q4 && K % 32 != 0))) return -1;
    // W as one tensor, or as three of N / 3 rows each, one behind the other (what a stacked Q | K | V matrix is made of)
    HostTensor part[3];
    std::vector<const HostTensor *> rows;
    const int n_parts = stack3 ? 3 : 1;
    for (int i = 0; form != 6 && i < n_parts; ++i) {
        HostTensor &t = part[i];
        t.type = wtype; t.n_dims = 2; t.ne0 = K; t.ne1 = N / n_parts;
        t.nbytes = wtype_row_bytes(wtype, K) * (size_t)t.ne1;
        t.data = (const uint8_t *)W + t.nbytes * i;
        rows.push_back(&t);
    }
    StackedRows s;
    std::string err;
    if (form != 6 && !s.stack(rows, err)) return -1;
    auto give = [&](const auto &v) -> int32_t {
        const size_t bytes = v.size() * sizeof(v[0]);
        if ((int64_t)bytes > out_cap) return -2;
        memcpy(out, v.data(), bytes);
        return (int32_t)bytes;
    };
    switch (form) {
        case 0: return give(pack_f16_image(s, s.N_pad));
        case 1: return K % 16 ? -1 : give(permute_k16(pack_f16_image(s, s.N_pad)));
        case 2: case 3: {
            if (!q4 || !s.mfma_ok) return -1;
            const Q4Planes pl = pack_q4_planes(s);
            return give(form == 2 ? pl.qs : pl.sc);
        }
        case 4: case 5: {
            if (!gamma || !beta) return -1;
            const LnFoldImage f = pack_ln_fold(s, gamma, beta, bias);
            return give(form == 4 ? f.img : f.aug);
        }
        case 6: return gamma && beta && bias ? give(pack_gamma_beta_bias(gamma, beta, bias, N)) : -1;
        case 7: return q4 && !stack3 ? give(table_as_f32(part[0])) : -1;
    }
    return -1;
}

void bert_hip_test_shard_bounds(const int32_t *cu_seqlens, int32_t n_sentences, int32_t n_shards, int32_t *bounds) {
    std::vector<int> b;
    shard_bounds(cu_seqlens, n_sentences, n_shards, b);
    for (size_t i = 0; i < b.size(); ++i) bounds[i] = b[i];
}

int32_t bert_hip_test_build_windows(const int32_t *cu_seqlens, int32_t n_sentences, int32_t *windows) {
    std::vector<int2> w;
    Engine::build_windows(cu_seqlens, n_sentences, w, window_slots());
    for (size_t i = 0; i < w.size(); ++i) { windows[2 * i] = w[i].x; windows[2 * i + 1] = w[i].y; }
    return (int32_t)w.size();
}

int32_t bert_hip_test_max_windows(int32_t n_sentences, int32_t n_tokens) { return qkv_attention2_max_windows(n_sentences, n_tokens, window_slots()); }

int32_t bert_hip_test_set_window_slots(int32_t slots) { set_window_slots(slots); return window_slots(); }

void bert_hip_test_set_pad(uint32_t pattern16, uint32_t pattern32) { g_pad16 = (uint16_t)pattern16; g_pad32 = pattern32; }

int32_t bert_hip_test_build_windows_device(const int32_t *cu_seqlens, int32_t n_sentences, int32_t *windows) {
    std::string err;
    DevBuf dcu, dwin, dcount;
    if (!dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * sizeof(int32_t), err) ||
        !dwin.alloc((size_t)std::max(n_sentences, 1) * sizeof(int2), err) || !dcount.alloc(sizeof(int), err)) return -1;
    launch_build_windows(dcu.as<int32_t>(), n_sentences, dwin.as<int2>(), dcount.as<int>(), window_slots(), nullptr);
    int n = -1;
    if (hipMemcpy(&n, dcount.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || n < 0 || n > n_sentences) return -1;
    if (n && hipMemcpy(windows, dwin.p, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}

int64_t bert_hip_test_shard_threads_created(void) { return (int64_t)ShardWorkers::threads_created(); }

int32_t bert_hip_test_dispatch(const bert_vocab_id *tokens, const int32_t *cu_seqlens, int32_t n_sentences, int32_t n_shards,
                               int32_t H, float *out) {
    std::vector<int> bounds;
    shard_bounds(cu_seqlens, n_sentences, n_shards, bounds);
    // one pool for the life of the process, like a context's (sized for the largest shard count seen so far)
    static std::unique_ptr<ShardWorkers> pool;
    if (!pool || pool->n_threads() < n_shards - 1) pool.reset(new ShardWorkers(n_shards - 1));
    return pool->run(bounds, [&](int shard, int b0, int b1) {
        if (H < 0) throw std::runtime_error("injected failure in shard " + std::to_string(shard));
        // stands in for Engine::eval_packed_host(tokens, cu + b0, b1 - b0, out + b0 * H): the global token array and a
        // window of the prefix sums, results into the caller's rows of this shard
        const int32_t *cu = cu_seqlens + b0;
        float *dst = out + (size_t)b0 * H;
        for (int b = 0; b < b1 - b0; ++b) {
            long long sum = 0;
            for (int t = cu[b]; t < cu[b + 1]; ++t) sum += tokens[t];
            for (int e = 0; e < H; ++e) dst[(size_t)b * H + e] = e == 0 ? (float)sum : e == 1 ? (float)(cu[b + 1] - cu[b]) : e == 2 ? (float)shard : (float)(b0 + b);
        }
        return 0;
    });
}

int32_t bert_hip_test_parse_devices(const char *list, int32_t n_devices, int32_t current, int32_t *devs, char *err, int32_t err_cap) {
    std::vector<int> d;
    std::string e;
    if (!parse_device_list(list, n_devices, current, d, e)) {
        snprintf(err, (size_t)err_cap, "%s", e.c_str());
        return -1;
    }
    for (size_t i = 0; i < d.size(); ++i) devs[i] = d[i];
    return (int32_t)d.size();
}

int32_t bert_hip_test_gather_runs(const int32_t *cu_seqlens, int32_t n_sentences, int64_t tokens_per_run, int32_t *runs) {
    std::vector<int> r;
    gather_runs(cu_seqlens, n_sentences, tokens_per_run, r);
    for (size_t i = 0; i < r.size(); ++i) runs[i] = r[i];
    return (int32_t)r.size();
}

int32_t bert_hip_test_encode_groups(int32_t n_inputs, int32_t *groups, int32_t cap) {
    int32_t k = 0;
    for (int32_t left = n_inputs; left > 0; ++k) {
        const int32_t n = encode_group_size(k, left);
        if (k < cap) groups[k] = n;
        left -= n;
    }
    return k;
}

int32_t bert_hip_test_tokenize_pack(struct bert_ctx *ctx, int32_t n_threads, int32_t n, const char **texts, const int32_t *counts,
                                    int32_t *n_tokens, int32_t *cu, bert_vocab_id *packed, int32_t packed_cap) {
    TokenGroup &g = ctx->texts.group[0];
    g.tokenize(ctx->texts, n_threads, n, texts);
    if (counts) {
        std::copy(counts, counts + n, g.n_tokens.begin());
        g.pack(ctx->texts.n_max_tokens, n);
    }
    if (g.cu[g.n_ok] > packed_cap) return -1;
    std::copy(g.n_tokens.begin(), g.n_tokens.end(), n_tokens);
    std::copy(g.cu.begin(), g.cu.begin() + g.n_ok + 1, cu);
    std::copy(g.packed.get(), g.packed.get() + g.cu[g.n_ok], packed);
    return g.n_ok;
}

int32_t bert_hip_test_index_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err, int32_t err_cap) {
    IndexFileHeader h;
    std::string e;
    if (err && err_cap > 0) err[0] = 0;
    if (buf_len < 0 || file_bytes < 0) e = "negative length";
    else if (index_header_check(buf, (size_t)buf_len, (uint64_t)file_bytes, h, e)) {
        const uint32_t f[6] = {h.version, h.dtype, h.dim, h.dpad, h.n_rows, h.has_live};
        if (fields) std::copy(f, f + 6, fields);
        return 0;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", e.c_str());
    return -1;
}

int32_t bert_hip_test_partition_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err, int32_t err_cap) {
    PartitionFileHeader h;
    std::string e;
    if (err && err_cap > 0) err[0] = 0;
    if (buf_len < 0 || file_bytes < 0) e = "negative length";
    else if (partition_header_check(buf, (size_t)buf_len, (uint64_t)file_bytes, h, e)) {
        const uint32_t f[4] = {h.version, h.dim, h.n_lists, h.n_part};
        if (fields) std::copy(f, f + 4, fields);
        return 0;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", e.c_str());
    return -1;
}

int32_t bert_hip_test_sparse_index_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err, int32_t err_cap) {
    SparseIndexFileHeader h;
    std::string e;
    if (err && err_cap > 0) err[0] = 0;
    if (buf_len < 0 || file_bytes < 0) e = "negative length";
    else if (sparse_index_header_check(buf, (size_t)buf_len, (uint64_t)file_bytes, h, e)) {
        const uint32_t f[6] = {h.version, h.dtype, h.n_vocab, h.width, h.n_rows, h.has_live};
        if (fields) std::copy(f, f + 6, fields);
        return 0;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", e.c_str());
    return -1;
}

int32_t bert_hip_test_sparse_index_body(const uint32_t *fields, const void *body, int64_t body_len, char *err, int32_t err_cap) {
    std::string e;
    if (err && err_cap > 0) err[0] = 0;
    if (!fields || body_len < 0) e = "fields and a body length >= 0 required";
    else {
        // (the fields through the header check itself: a body is only ever checked under a header that passed)
        SparseIndexFileHeader g, h;
        g.version = fields[0]; g.dtype = fields[1]; g.n_vocab = fields[2]; g.width = fields[3]; g.n_rows = fields[4]; g.has_live = fields[5];
        unsigned char hdr[INDEX_HEADER_BYTES];
        sparse_index_header_write(g, hdr);
        if (sparse_index_header_check(hdr, sizeof hdr, (uint64_t)body_len + INDEX_HEADER_BYTES, h, e) && sparse_index_body_check(h, body, (uint64_t)body_len, e)) return 0;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", e.c_str());
    return -1;
}

int32_t bert_hip_test_late_index_header(const void *buf, int32_t buf_len, int64_t file_bytes, uint32_t *fields, char *err, int32_t err_cap) {
    TokenIndexFileHeader h;
    std::string e;
    if (err && err_cap > 0) err[0] = 0;
    if (buf_len < 0 || file_bytes < 0) e = "negative length";
    else if (token_index_header_check(buf, (size_t)buf_len, (uint64_t)file_bytes, h, e)) {
        const uint32_t f[6] = {h.version, h.dim, h.n_docs, h.has_live, (uint32_t)h.n_tokens, (uint32_t)(h.n_tokens >> 32)};
        if (fields) std::copy(f, f + 6, fields);
        return 0;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", e.c_str());
    return -1;
}

int32_t bert_hip_test_late_index_body(const uint32_t *fields, const void *body, int64_t body_len, char *err, int32_t err_cap) {
    std::string e;
    if (err && err_cap > 0) err[0] = 0;
    if (!fields || body_len < 0) e = "fields and a body length >= 0 required";
    else {
        // (the fields through the header check itself: a body is only ever checked under a header that passed)
        TokenIndexFileHeader g, h;
        g.version = fields[0]; g.dim = fields[1]; g.n_docs = fields[2]; g.has_live = fields[3]; g.n_tokens = (uint64_t)fields[4] | (uint64_t)fields[5] << 32;
        unsigned char hdr[INDEX_HEADER_BYTES];
        token_index_header_write(g, hdr);
        if (token_index_header_check(hdr, sizeof hdr, (uint64_t)body_len + INDEX_HEADER_BYTES, h, e) && token_index_body_check(h, body, (uint64_t)body_len, e)) return 0;
    }
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", e.c_str());
    return -1;
}

int32_t bert_hip_test_build_lists(const int32_t *list_of, int32_t n, int32_t n_lists, int32_t *offsets, int32_t *order) {
    if (n < 0 || n_lists < 0 || (n > 0 && !list_of) || !offsets || (n > 0 && !order)) return -1;
    ListTables t;
    build_lists(list_of, n, n_lists, t);
    std::copy(t.offsets.begin(), t.offsets.end(), offsets);
    std::copy(t.order.begin(), t.order.end(), order);
    return (int32_t)t.order.size();
}

int32_t bert_hip_test_token_rows(const void *x, int32_t is_f32, int32_t T, int32_t H, const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len,
                                 int32_t flags, void *out) {
    const char *me = "bert_hip_test_token_rows";
    if (!x || !cu_seqlens || !out || T < 1 || H < 1 || n_sentences < 1 || (flags & ~3)) return -1;
    std::string err;
    const int T_pad = (T + GEMM_BM - 1) / GEMM_BM * GEMM_BM;
    const bool o16 = flags & TOKEN_ROWS_F16;
    DevBuf dx, dcu, dout;
    const bool ok = (is_f32 ? upload_padded(dx, (const uint32_t *)x, T, T_pad, H, g_pad32, err) : upload_rows16(dx, (const uint16_t *)x, T, T_pad, H, err)) &&
                    dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) &&
                    (o16 ? alloc_pad16(dout, (size_t)T * H, err) : alloc_pad32(dout, (size_t)T * H, err));
    if (!ok) { fprintf(stderr, "%s: %s\n", me, err.c_str()); return -1; }
    launch_token_rows(dx.p, is_f32 != 0, T, H, dcu.as<int32_t>(), n_sentences, max_len, flags, dout.p, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dout.p, (size_t)T * H * (o16 ? 2 : 4), hipMemcpyDeviceToHost));
    return 0;
}

int32_t bert_hip_test_embed_ln_typed(int32_t table_type, int32_t H, int32_t n_vocab, int32_t n_pos, const void *word, const void *type,
                                     const void *pos, const float *gamma, const float *beta, const bert_vocab_id *tokens,
                                     const int32_t *cu_seqlens, int32_t n_sentences, int32_t max_len, const int32_t *first_len, int32_t form,
                                     void *out) {
    const char *me = "bert_hip_test_embed_ln_typed";
    std::string err;
    if (H <= 0 || n_vocab <= 0 || n_sentences <= 0 || max_len < 0 || max_len > n_pos || form < 0 || form > 4 || table_type < 0 || table_type > 3) return -1;
    if (form == 4 && table_type != W_F32) return -2;
    const int T = cu_seqlens[n_sentences], T_pad = form == 4 ? f32_rows_pad(T) : rows_pad256(T);
    if (max_len == 0)
        for (int b = 0; b < n_sentences; ++b) max_len = std::max(max_len, cu_seqlens[b + 1] - cu_seqlens[b]);
    if (max_len > n_pos || max_len <= 0) return -1;
    if (form == 3 && !embed_ln_lanes_supported(table_type, H, T, max_len)) return -2;
    const size_t rb = wtype_row_bytes(table_type, H);
    DevBuf dw, dt, dp, dg, db, dtok, dcu, dfl, dout;
    if (!dw.upload(word, rb * n_vocab, err) || !dt.upload(type, rb * 2, err) || !dp.upload(pos, rb * n_pos, err) ||
        !dg.upload(gamma, (size_t)H * 4, err) || !db.upload(beta, (size_t)H * 4, err) || !dtok.upload(tokens, (size_t)T * 4, err) ||
        !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) || (first_len && !dfl.upload(first_len, (size_t)n_sentences * 4, err)) ||
        !(form == 4 ? alloc_pad32(dout, (size_t)T_pad * H, err) : alloc_pad16(dout, (size_t)T_pad * H, err))) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    const int32_t *fl = first_len ? dfl.as<int32_t>() : nullptr;
    bool launched = true;
    if (form == 4)
        launch_f32_embed_ln(dw.as<float>(), dt.as<float>(), dp.as<float>(), dg.as<float>(), db.as<float>(), dtok.as<int32_t>(), dcu.as<int32_t>(), n_sentences, T,
                            H, n_vocab, max_len, dout.as<float>(), nullptr, fl);
    else if (form == 3)
        launched = launch_embed_ln_lanes(dw.p, dt.p, dp.p, table_type, dg.as<float>(), db.as<float>(), dtok.as<int32_t>(), dcu.as<int32_t>(), n_sentences, T, H,
                                         n_vocab, max_len, dout.as<half_t>(), nullptr, fl);
    else
        launched = launch_embed_ln(dw.p, dt.p, dp.p, table_type, dg.as<float>(), db.as<float>(), dtok.as<int32_t>(), dcu.as<int32_t>(), n_sentences, T, H, n_vocab,
                                   max_len, dout.as<half_t>(), nullptr, fl, form);
    if (!launched) return -2;
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return form == 4 ? download_rows32(me, (float *)out, dout, T, T_pad, H) : download_rows16(me, (uint16_t *)out, dout, T, T_pad, H);
}

int32_t bert_hip_test_cls_head(int32_t B, int32_t H, int32_t n_labels, const float *rows, const void *Wp, int32_t wp_is_f32, const float *bp,
                               const float *Wc, const float *bc, int32_t flags, int32_t form, float *out) {
    const char *me = "bert_hip_test_cls_head";
    if (B < 1 || H < 1 || n_labels < 1 || n_labels > CLS_HEAD_MAX_LABELS || !rows || !Wp || !bp || !Wc || !bc || !out || (flags & ~1) || form < 0 || form > 1) return -1;
    if (form == 0 && (wp_is_f32 || !cls_head_mfma_supported(H))) return -2;
    std::string err;
    // the rows as the engine's d_out_ holds them, one more block of 32 sentences behind the last whole one: those hold the 32-bit pattern,
    // as every word of the output does before the launch
    const int B_pad = (B + 31) / 32 * 32 + 32;
    DevBuf drows, dwp, dbp, dwc, dbc, dout;
    if (!upload_padded(drows, (const uint32_t *)rows, B, B_pad, H, g_pad32, err) || !dwp.upload(Wp, (size_t)H * H * (wp_is_f32 ? 4 : 2), err) ||
        !dbp.upload(bp, (size_t)H * 4, err) || !dwc.upload(Wc, (size_t)n_labels * H * 4, err) || !dbc.upload(bc, (size_t)n_labels * 4, err) ||
        !alloc_pad32(dout, (size_t)B_pad * n_labels, err)) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    const ClsHeadArgs a{drows.as<float>(), wp_is_f32 ? nullptr : dwp.as<half_t>(), wp_is_f32 ? dwp.as<float>() : nullptr, dbp.as<float>(), dwc.as<float>(),
                        dbc.as<float>(), dout.as<float>(), B, H, n_labels, flags};
    if (!(form == 0 ? launch_cls_head(a, nullptr) : launch_cls_head_f32(a, nullptr))) return -2;
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> h((size_t)B_pad * n_labels);
    CK(hipMemcpy(h.data(), dout.p, h.size() * 4, hipMemcpyDeviceToHost));
    memcpy(out, h.data(), (size_t)B * n_labels * 4);
    for (size_t i = (size_t)B * n_labels; i < h.size(); ++i)
        if (h[i] != g_pad32) { fprintf(stderr, "%s: a score behind the last sentence was written\n", me); return -4; }
    return 0;
}

int32_t bert_hip_test_sparse_vocab(int32_t form, int32_t H, int32_t V, const void *t, int32_t t_is_f32, const void *e, int32_t e_is_f32,
                                   const float *bias, const int32_t *cu_seqlens, int32_t n_sentences, int32_t s0, int32_t ns, float *out) {
    const char *me = "bert_hip_test_sparse_vocab";
    if (form < 0 || form > 1 || H < 1 || V < 1 || !t || !e || !bias || !cu_seqlens || n_sentences < 1 || s0 < 0 || ns < 1 || s0 + ns > n_sentences || !out) return -1;
    if (form == 0 && (t_is_f32 || e_is_f32 || !sparse_vocab_mfma_supported(H))) return -2;
    std::string err;
    const int T = cu_seqlens[n_sentences], GUARD = 64;
    int max_len = 1;
    for (int b = s0; b < s0 + ns; ++b) max_len = std::max(max_len, cu_seqlens[b + 1] - cu_seqlens[b]);
    if (T < 1) return -1;
    // NaN rows in front of and behind the token rows and behind the vocabulary image; the output holds negative, NaN and huge bit patterns,
    // with one row of pattern32 behind it
    const size_t ts = t_is_f32 ? 4 : 2, es = e_is_f32 ? 4 : 2;
    std::vector<uint8_t> ht((size_t)(T + 2 * GUARD) * H * ts, 0xFF), he((size_t)(V + GUARD) * H * es, 0xFF);      // (all ones: a NaN in f16 and in f32)
    memcpy(ht.data() + (size_t)GUARD * H * ts, t, (size_t)T * H * ts);
    memcpy(he.data(), e, (size_t)V * H * es);
    static const uint32_t garbage[4] = {0xFFC00001u, 0xBF800000u, 0x7FC00000u, 0x7F7FFFFFu};
    std::vector<uint32_t> ho((size_t)(ns + 1) * V);
    for (size_t i = 0; i < ho.size(); ++i) ho[i] = i < (size_t)ns * V ? garbage[i & 3] : g_pad32;
    DevBuf dt, de, db, dcu, dout;
    if (!dt.upload(ht, err) || !de.upload(he, err) || !db.upload(bias, (size_t)V * 4, err) || !dcu.upload(cu_seqlens, (size_t)(n_sentences + 1) * 4, err) ||
        !dout.upload(ho, err)) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    const char *tp = dt.as<char>() + (size_t)GUARD * H * ts;
    const SparseVocabArgs a{t_is_f32 ? nullptr : (const half_t *)tp, e_is_f32 ? nullptr : de.as<half_t>(), t_is_f32 ? (const float *)tp : nullptr,
                            e_is_f32 ? de.as<float>() : nullptr, db.as<float>(), dcu.as<int32_t>(), dout.as<float>(), s0, ns, T, H, V, max_len};
    if (form == 0) {
        if (!launch_sparse_vocab(a, nullptr)) return -2;
        launch_sparse_finish(dout.as<float>(), (size_t)ns * V, nullptr);
    } else if (!launch_sparse_vocab_f32(a, nullptr)) return -2;
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(ho.data(), dout.p, ho.size() * 4, hipMemcpyDeviceToHost));
    memcpy(out, ho.data(), (size_t)ns * V * 4);
    for (size_t i = (size_t)ns * V; i < ho.size(); ++i)
        if (ho[i] != g_pad32) { fprintf(stderr, "%s: a weight behind the last sentence was written\n", me); return -4; }
    return 0;
}

int32_t bert_hip_test_sparse_topk(const float *w, int32_t n, int32_t V, int32_t k, int32_t *ids, float *weights) {
    const char *me = "bert_hip_test_sparse_topk";
    if (!w || n < 1 || V < 1 || k < 1 || !ids || !weights) return -1;
    std::string err;
    DevBuf dw, di, dv;
    if (!dw.upload(w, (size_t)n * V * 4, err) || !alloc_pad32(di, (size_t)(n + 1) * k, err) || !alloc_pad32(dv, (size_t)(n + 1) * k, err)) {
        fprintf(stderr, "%s: %s\n", me, err.c_str());
        return -1;
    }
    if (!launch_sparse_topk(dw.as<float>(), n, V, k, di.as<int32_t>(), dv.as<float>(), nullptr)) return -2;
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<uint32_t> hi((size_t)(n + 1) * k), hv(hi.size());
    CK(hipMemcpy(hi.data(), di.p, hi.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv.data(), dv.p, hv.size() * 4, hipMemcpyDeviceToHost));
    memcpy(ids, hi.data(), (size_t)n * k * 4);
    memcpy(weights, hv.data(), (size_t)n * k * 4);
    for (size_t i = (size_t)n * k; i < hi.size(); ++i)
        if (hi[i] != g_pad32 || hv[i] != g_pad32) { fprintf(stderr, "%s: a place behind the last row was written\n", me); return -4; }
    return 0;
}

int32_t bert_hip_test_sparse_vocab_geometry(int32_t H, int32_t V, int32_t T, int32_t ns, int32_t max_len, int32_t *geometry) {
    if (!geometry) return -1;
    SparseVocabGeometry g;
    const bool ok = sparse_vocab_geometry(H, V, T, ns, max_len, g);
    geometry[0] = g.tile; geometry[1] = g.n_tiles; geometry[2] = g.slab_blocks; geometry[3] = g.n_slabs;
    return ok ? 0 : -2;
}

int32_t bert_hip_test_sparse_scan_geometry(int32_t dtype, int32_t n_vocab, int32_t n_rows, int32_t nq, int32_t k, int64_t *geometry) {
    if (!geometry) return -1;
    SparseScanGeometry g;
    const bool ok = sparse_scan_geometry(dtype, n_vocab, n_rows, nq, k, g);
    geometry[0] = g.qb; geometry[1] = g.n_qtiles; geometry[2] = g.n_slices; geometry[3] = g.slice_rows; geometry[4] = g.L; geometry[5] = (int64_t)g.lds;
    return ok ? 0 : -2;
}

int32_t bert_hip_test_sparse_scan_geometry_qb(int32_t dtype, int32_t n_vocab, int32_t n_rows, int32_t nq, int32_t k, int32_t qb, int64_t *geometry) {
    if (!geometry) return -1;
    SparseScanGeometry g;
    const bool ok = sparse_scan_geometry(dtype, n_vocab, n_rows, nq, k, g, qb);
    geometry[0] = g.qb; geometry[1] = g.n_qtiles; geometry[2] = g.n_slices; geometry[3] = g.slice_rows; geometry[4] = g.L; geometry[5] = (int64_t)g.lds;
    return ok ? 0 : -2;
}

int32_t bert_hip_test_sparse_postings_geometry(int32_t dtype, int32_t n_vocab, int32_t n_rows, int32_t nq, int32_t k, int32_t seg, int32_t qb,
                                               int64_t *geometry) {
    if (!geometry) return -1;
    SparsePostingsGeometry g;
    const bool ok = sparse_postings_geometry(dtype, n_vocab, n_rows, nq, k, seg, g, qb);
    geometry[0] = g.qb; geometry[1] = g.n_qtiles; geometry[2] = g.n_slices; geometry[3] = g.slice_segs; geometry[4] = g.L; geometry[5] = g.max_slices;
    geometry[6] = (int64_t)g.lds;
    return ok ? 0 : -2;
}

int32_t bert_hip_test_sparse_postings_segment(struct bert_hip_sparse_index *ix, int32_t segment, int32_t cap, uint32_t *off, int32_t *rows,
                                              float *weights, int32_t *seg_rows) {
    if (!ix || !ix->ix || !off || !rows || !weights || !seg_rows || cap < 0) return -1;
    std::vector<uint32_t> o;
    std::vector<uint16_t> r;
    std::vector<float> w;
    std::string err;
    const int total = ix->ix->postings_segment_host(segment, o, r, w, err);
    if (total < 0) return total;
    *seg_rows = ix->ix->segment_rows();
    memcpy(off, o.data(), o.size() * 4);
    for (int i = 0; i < std::min(total, cap); ++i) { rows[i] = r[(size_t)i]; weights[i] = w[(size_t)i]; }
    return total;
}

int32_t bert_hip_test_hybrid_chunk(int32_t n_rows, int32_t nq, int32_t pref, int64_t *out) {
    if (!out) return -1;
    out[0] = out[1] = 0;
    if (n_rows < 0 || nq < 1 || pref < 0) return -2;
    out[0] = hybrid_chunk_queries(n_rows, nq, pref);
    out[1] = (int64_t)hybrid_ld(n_rows);
    return 0;
}

int32_t bert_hip_test_token_index_plan(int32_t n_docs, int32_t nq, int32_t pref, int32_t *plan) {
    if (!plan) return -1;
    TokenScanPlan p;
    const bool ok = token_index_plan(n_docs, nq, pref, p);
    plan[0] = p.n_slices; plan[1] = p.slice_docs;
    return ok ? 0 : -2;
}

int32_t bert_hip_test_index_plan(int32_t n_rows, int32_t nq, int32_t k, int32_t *geometry) {
    if (!geometry) return -1;
    geometry[0] = geometry[1] = geometry[2] = geometry[3] = 0;
    if (n_rows < 0 || nq < 1 || nq > Index::QCHUNK || k < 1 || k > Index::MAX_K) return -2;
    int g[4];
    index_search_plan(n_rows, nq, k, g);
    for (int i = 0; i < 4; ++i) geometry[i] = g[i];
    return 0;
}

int32_t bert_hip_test_attention_grid(int32_t n_sentences, int32_t n_head, int32_t d_head, int32_t max_len, int32_t *threads, int32_t *items) {
    if (n_sentences < 1 || n_head < 1 || max_len < 1 || !threads || !items) return -1;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) { fprintf(stderr, "bert_hip_test_attention_grid: no device\n"); return -1; }
    const AttentionGrid g = attention_mfma_grid(n_sentences, n_head, d_head, max_len);
    *threads = g.threads; *items = g.items;
    return g.grid;
}

}  // extern "C"
