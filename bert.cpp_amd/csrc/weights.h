// weights.h — the weights of a model on the device: file tensors (model_file.h) repacked into the HBM layouts of kernels.h.
// Every image is made in two steps: a pure host function (pack_*, table_as_f32: bytes in, bytes out, nothing of HIP, checked
// bit for bit on the CPU by tests/test_pack_host.py) and an upload.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"
#include "model_file.h"

namespace bert_hip {

#define HIP_OK(expr, errvar, ret)                                                                       \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            errvar = std::string(#expr) + ": " + hipGetErrorString(e__);                                \
            return ret;                                                                                 \
        }                                                                                               \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf();
    bool alloc(size_t n, std::string &err);                       // zero-filled
    bool upload(const void *src, size_t n, std::string &err);     // alloc + H2D
    template <class T> bool upload(const std::vector<T> &v, std::string &err) { return upload(v.data(), v.size() * sizeof(T), err); }
    bool ensure(size_t n, std::string &err);                      // grow only
    template <class T> T *as() const { return (T *)p; }
};

// ------------------------------------------------------------------------------------------------
// packing (host only)
// ------------------------------------------------------------------------------------------------

// File tensors stacked along N (one entry, or q|k|v; all share type and K) seen as one matrix W[N][K]: its sizes, whether the
// MFMA kernels take it, and the walk over its rows.
struct StackedRows {
    std::vector<const HostTensor *> parts;
    int64_t N = 0, K = 0, N_pad = 0;      // N_pad: whole GEMM_BN tiles
    int32_t type = W_F32;
    bool mfma_ok = false;
    bool stack(const std::vector<const HostTensor *> &rows, std::string &err);
    bool q4() const { return type == W_Q4_0 || type == W_Q4_1; }
    size_t row_bytes() const { return wtype_row_bytes(type, K); }
    template <class F> void for_each_row(F &&f) const {          // f(n, the file bytes of row n)
        int64_t n = 0;
        for (auto *t : parts)
            for (int64_t r = 0; r < t->ne1; ++r, ++n) f(n, t->data + row_bytes() * (size_t)r);
    }
};

// A q4_0 / q4_1 block of the file (18 / 20 bytes): scale, minimum (0 for q4_0) and the 32 4-bit values in element order
// (byte j of the block holds elements j and j + 16).  The one reader of the format on the host.
struct Q4Block { float d, m; uint8_t q[32]; };
Q4Block read_q4_block(int32_t type, const uint8_t *blk);

// one row of a file tensor as f16: exactly representable for f16 files, nearest for f32 / q4.  For q4 these are the bits the
// fused-dequant kernels build in registers (device.h), so they are the definition of a q4 weight's value.
void row_to_f16(int32_t type, int64_t K, const uint8_t *src, _Float16 *dst);

// GW_F16 image [n_rows][K] row-major, rows from N on zero (n_rows: N_pad, or N for GemmWeight::naive16)
std::vector<_Float16> pack_f16_image(const StackedRows &s, int64_t n_rows);
// GemmWeight::w16p: position j of every group of 16 holds k offset [0-3, 8-11, 4-7, 12-15][j]
std::vector<_Float16> permute_k16(const std::vector<_Float16> &img);
// GW_Q4_x planes: 16 bytes of nibbles / the f16 scale (q4_0) or {scale, minimum} (q4_1) per block, tile-contiguous (kernels.h)
struct Q4Planes { std::vector<uint8_t> qs, sc; };
Q4Planes pack_q4_planes(const StackedRows &s);
// LayerNorm folded into a mat-mul that consumes LayerNorm(u; gamma, beta) (kernels.h GemmLnFold): img = the f16 image of
// W diag(gamma), [N_pad][K]; aug = the weight side of the statistics k-step, [N][16] f16: s_hi s_lo s_hi c_hi c_lo c_hi 0..
// with s[n] = sum_k W'[n][k], c[n] = sum_k beta[k] W[n][k] + bias[n] (bias may be null), summed in double in index order
struct LnFoldImage { std::vector<_Float16> img, aug; };
LnFoldImage pack_ln_fold(const StackedRows &s, const float *gamma, const float *beta, const float *bias);
// (f16 gamma | f16 (beta + bias) << 16) per feature: what a residual mat-mul needs to rebuild LayerNorm(resid) per element
std::vector<uint32_t> pack_gamma_beta_bias(const float *gamma, const float *beta, const float *bias, int64_t n);
// an embedding table of a q4 file as f32 values, the numbers the gather kernel dequantises on the fly
std::vector<float> table_as_f32(const HostTensor &t);
// any file tensor as f32 values [ne1][ne0]: f32 as stored, f16 widened, q4 as table_as_f32
std::vector<float> tensor_as_f32(const HostTensor &t);
// MPNet's relative position bucket of the distance d = key - query (MPNetEncoder.relative_position_bucket with 32 buckets and
// max_distance 128, in integers): keys behind the query take buckets 16 .. 31, distances below 8 a bucket each, the larger ones the
// log-spaced ranges that start at 8, 12, 16, 23, 32, 46, 64 and 91
int rel_bias_bucket(int d);
// the bias of every distance a sentence of up to P tokens can hold: W [REL_BUCKETS][n_head] f32 -> rel [n_head][2 P - 1] with
// rel[h][d + P - 1] = W[rel_bias_bucket(d)][h] * scale, the product rounded once to f32 (scale 1: W's own values)
std::vector<float> rel_bias_table(const float *W, int n_head, int P, double scale);

// ------------------------------------------------------------------------------------------------
// images on the device
// ------------------------------------------------------------------------------------------------
struct PackOptions {
    bool naive = false;        // also GemmWeight::naive16 (built anyway for shapes the MFMA kernels do not take)
    bool kperm = false;        // also GemmWeight::w16p (f16 images only)
    bool expand_q4 = false;    // q4_0 / q4_1 tensors become an f16 image at load (the engine's default) instead of the nibble /
                               // scale planes of the fused-dequant kernels
    bool f32 = false;          // f32 tensors also keep their own f32 rows (GemmWeight::w32, the f32 route)
};

// Owns the HBM image of one weight matrix in the layouts kernels.h describes.
struct GemmWeightStore {
    GemmWeight w;
    DevBuf w16, w16p, qs, sc, naive16, w32;
    bool mfma_ok = false;
    // rows: file tensors stacked along N (StackedRows)
    bool build(const std::vector<const HostTensor *> &rows, const PackOptions &opt, std::string &err);
    // pack_ln_fold: the image in this store, the statistics columns in waug
    bool build_ln_fold(const std::vector<const HostTensor *> &rows, const float *gamma, const float *beta, const float *bias, DevBuf &waug, std::string &err);
};

struct LayerWeights {
    GemmWeightStore qkv, o, ffi, ffo;
    // q4 files with the default BERT_HIP_Q4=expand: the stacked Q | K | V matrix ALSO as 4-bit planes when its f16 image
    // (3 H x H x 2 bytes) cannot stay in an XCD's 4 MiB L2 beside the activation tiles in flight — gemm256's persistent walk
    // then re-fetches the f16 image every round (2.40 GB per launch at bert-base dims against 0.81 GB with the planes, which
    // give the same bits and are 1-3 % faster on that launch: DESIGN.md §3).  Used by the QKV mat-mul of the gemm256 route only.
    GemmWeightStore qkv_q4;
    DevBuf qkv_b, o_b, ffi_b, ffo_b, ln_att_w, ln_att_b, ln_out_w, ln_out_b;
    // LayerNorm folded into the H = 768 mat-muls (kernels.h GemmLnFold): the up-projection with this layer's attention LayerNorm
    // folded in, the Q|K|V projection with the PREVIOUS layer's output LayerNorm (layers >= 1), their statistics columns, and
    // the packed (gamma, beta + bias) pairs of the two residual mat-muls (attention output: the previous layer's output LayerNorm)
    GemmWeightStore ffi_fold, qkv_fold;
    DevBuf ffi_waug, qkv_waug, o_gb, ffo_gb;
    bool fold_ok = false;
};

// what is decided once, when the weights are packed (no option can change it later)
struct LoadOptions {
    bool naive = false;        // the f16 row-major images of the generic kernels for every matrix
    bool expand_q4 = true;     // q4 files: f16 images and f32 tables, else the 4-bit planes and the file's own tables
    bool ln_fold = true;       // the LayerNorm-folding images of models the fused H <= 384 kernels do not take
};

struct ModelWeights {
    int table_type = 0;                   // WType of the three embedding tables as uploaded
    DevBuf word_emb, type_emb, pos_emb, ln_e_w, ln_e_b;
    std::vector<LayerWeights> layers;
    bool f32_file = false;                // every matrix and table of the file is f32: the f32 route can take it
    bool fold_images = false;             // the LayerNorm-folding images were built (LoadOptions::ln_fold)
    bool naive_images() const;            // every matrix has GemmWeight::naive16
    // The classification head of the file, if it has one (model_file.h; cls_head.hip): Wp [H][H] as f16 (the file's f16 bits, or its
    // f32 / q4 values rounded once: row_to_f16), and for f32 files also its own f32 rows (the f32 route); bp [H], Wc [n_labels][H],
    // bc [n_labels] as f32 (q4 / f16 classifiers dequantised at load).  n_labels == 0: no head, nothing uploaded.
    int n_labels = 0;
    DevBuf head_wp16, head_wp32, head_bp, head_wc, head_bc;
    // The masked-language-model head of the file, if it has one (model_file.h; sparse_vocab.hip): the transform matrix as a layer's
    // matrices are (f32 files also keep its f32 rows), its bias, the transform's LayerNorm and the output bias [n_vocab] as f32, and the
    // tied vocabulary matrix as an f16 image [n_vocab][H]: for f16 files word_emb itself, no second copy; for q4 and f32 files one
    // rounding per element (row_to_f16) into vocab16_own, made only when the head is present.
    bool mlm_head = false;
    GemmWeightStore mlm_wt;
    DevBuf mlm_bt, mlm_ln_w, mlm_ln_b, mlm_bias, vocab16_own;
    const half_t *vocab16 = nullptr;
    // The relative position bias of the file, if it has one (model_file.h; attention.hip, f32_route.hip): rel_bias_table for
    // P = n_max_tokens, as the kernels that scale a score themselves add it (rel) and times sqrt(d_head) for the matrix-core kernel,
    // which scales the sum (rel_scaled).  One table for all layers.
    bool rel_bias = false;
    DevBuf rel, rel_scaled;
    // uploads to the current device
    static std::unique_ptr<ModelWeights> load(const ModelFile &mf, const LoadOptions &opt, std::string &err);
};

}  // namespace bert_hip
