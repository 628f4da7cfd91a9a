// weights.cpp — see weights.h.
#include "weights.h"

#include <cmath>
#include <cstring>

namespace bert_hip {

// ------------------------------------------------------------------------------------------------
// DevBuf
// ------------------------------------------------------------------------------------------------
DevBuf::~DevBuf() {
    if (p) (void)hipFree(p);
}
bool DevBuf::alloc(size_t n, std::string &err) {
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    if (n == 0) n = 16;
    HIP_OK(hipMalloc(&p, n), err, false);
    bytes = n;
    HIP_OK(hipMemset(p, 0, n), err, false);
    // the fill runs on the null stream and returns early; the engine's streams are non-blocking (not ordered
    // against it), so a kernel writing this buffer could be overtaken by the fill
    HIP_OK(hipDeviceSynchronize(), err, false);
    return true;
}
bool DevBuf::upload(const void *src, size_t n, std::string &err) {
    if (!alloc(n, err)) return false;
    if (n) HIP_OK(hipMemcpy(p, src, n, hipMemcpyHostToDevice), err, false);
    return true;
}
bool DevBuf::ensure(size_t n, std::string &err) {
    if (n <= bytes) return true;
    return alloc(n + n / 8, err);
}

// ------------------------------------------------------------------------------------------------
// packing (host only): file tensors -> the bytes of the HBM layouts of kernels.h
// ------------------------------------------------------------------------------------------------
bool StackedRows::stack(const std::vector<const HostTensor *> &rows, std::string &err) {
    parts = rows;
    K = rows[0]->ne0; type = rows[0]->type; N = 0;
    for (auto *t : rows) {
        if (t->ne0 != K || t->type != type) { err = "stacked weights disagree in shape/type"; return false; }
        N += t->ne1;
    }
    N_pad = (N + GEMM_BN - 1) / GEMM_BN * GEMM_BN;
    mfma_ok = (K % GEMM_BK == 0) && (N % 8 == 0);
    return true;
}

static inline float h2f(const uint8_t *bits) { _Float16 h; memcpy(&h, bits, 2); return (float)h; }

Q4Block read_q4_block(int32_t type, const uint8_t *blk) {
    Q4Block b;
    b.d = h2f(blk);
    b.m = type == W_Q4_1 ? h2f(blk + 2) : 0.f;
    const uint8_t *qs = blk + (type == W_Q4_1 ? 4 : 2);
    for (int j = 0; j < 16; ++j) { b.q[j] = qs[j] & 0x0F; b.q[j + 16] = qs[j] >> 4; }
    return b;
}

void row_to_f16(int32_t type, int64_t K, const uint8_t *src, _Float16 *dst) {
    if (type == W_F32) {
        const float *f = (const float *)src;
        for (int64_t k = 0; k < K; ++k) dst[k] = (_Float16)f[k];
    } else if (type == W_F16) {
        memcpy(dst, src, (size_t)K * 2);
    } else {
        const size_t bs = wtype_row_bytes(type, 32);
        for (int64_t b = 0; b < K / 32; ++b) {
            const Q4Block blk = read_q4_block(type, src + b * bs);
            // q4_1 in double (q d + m is exact there): ONE rounding to f16, like the f16 fma of the fused-dequant kernels
            for (int j = 0; j < 32; ++j)
                dst[b * 32 + j] = type == W_Q4_0 ? (_Float16)((float)(blk.q[j] - 8) * blk.d) : (_Float16)((double)blk.q[j] * blk.d + blk.m);
        }
    }
}

std::vector<float> table_as_f32(const HostTensor &t) {
    const int64_t K = t.ne0, N = t.ne1;
    const size_t bs = wtype_row_bytes(t.type, 32), rb = wtype_row_bytes(t.type, K);
    std::vector<float> img((size_t)N * K);
    for (int64_t r = 0; r < N; ++r)
        for (int64_t b = 0; b < K / 32; ++b) {
            const Q4Block blk = read_q4_block(t.type, t.data + rb * (size_t)r + b * bs);
            float *dst = img.data() + (size_t)r * K + b * 32;
            // in f32, as the gather kernel does it (q d is exact in f32, so the host's multiply-add and the device's fma round
            // alike): not the f16 value of row_to_f16
            for (int j = 0; j < 32; ++j) dst[j] = t.type == W_Q4_0 ? (float)(blk.q[j] - 8) * blk.d : (float)blk.q[j] * blk.d + blk.m;
        }
    return img;
}

std::vector<float> tensor_as_f32(const HostTensor &t) {
    if (t.type == W_Q4_0 || t.type == W_Q4_1) return table_as_f32(t);
    const size_t n = (size_t)t.ne0 * t.ne1;
    std::vector<float> v(n);
    if (t.type == W_F32) memcpy(v.data(), t.data, n * 4);
    else
        for (size_t i = 0; i < n; ++i) { _Float16 h; memcpy(&h, t.data + 2 * i, 2); v[i] = (float)h; }
    return v;
}

int rel_bias_bucket(int d) {
    static const int thr[8] = {8, 12, 16, 23, 32, 46, 64, 91};
    const int m = d < 0 ? -d : d, base = d > 0 ? REL_BUCKETS / 2 : 0;
    if (m < 8) return base + m;
    int t = 0;
    while (t + 1 < 8 && thr[t + 1] <= m) ++t;
    return base + 8 + t;
}

std::vector<float> rel_bias_table(const float *W, int n_head, int P, double scale) {
    const int L = 2 * P - 1;
    std::vector<float> rel((size_t)n_head * L);
    for (int h = 0; h < n_head; ++h)
        for (int d = -(P - 1); d <= P - 1; ++d) rel[(size_t)h * L + d + P - 1] = (float)((double)W[(size_t)rel_bias_bucket(d) * n_head + h] * scale);
    return rel;
}

std::vector<_Float16> pack_f16_image(const StackedRows &s, int64_t n_rows) {
    std::vector<_Float16> img((size_t)n_rows * s.K, (_Float16)0);
    s.for_each_row([&](int64_t n, const uint8_t *src) { row_to_f16(s.type, s.K, src, img.data() + (size_t)n * s.K); });
    return img;
}

std::vector<_Float16> permute_k16(const std::vector<_Float16> &img) {
    std::vector<_Float16> pimg(img.size());
    for (size_t base = 0; base < img.size(); base += 16)
        for (int j = 0; j < 16; ++j) {
            // stored position j of a group <- k offset: [0-3, 8-11, 4-7, 12-15]
            const int src = (j & 3) + ((j >> 2) & 1) * 8 + (j >> 3) * 4;
            pimg[base + j] = img[base + src];
        }
    return pimg;
}

Q4Planes pack_q4_planes(const StackedRows &s) {
    const size_t scb = s.type == W_Q4_0 ? 2 : 4, bs = scb + 16;
    const int64_t nkt = s.K / GEMM_BK;
    const size_t nblk = (size_t)(s.N_pad / GEMM_BN) * nkt * 256;
    Q4Planes pl{std::vector<uint8_t>(nblk * 16, 0), std::vector<uint8_t>(nblk * scb, 0)};
    s.for_each_row([&](int64_t n, const uint8_t *src) {
        const int64_t nt = n / 128, row = n % 128;
        for (int64_t b = 0; b < s.K / 32; ++b) {
            const uint8_t *blk = src + (size_t)b * bs;
            const size_t bi = ((size_t)(nt * nkt + b / 2) * 128 + row) * 2 + b % 2;
            memcpy(pl.sc.data() + bi * scb, blk, scb);                   // d  or  {d, m}
            memcpy(pl.qs.data() + bi * 16, blk + scb, 16);               // 32 nibbles
        }
    });
    return pl;
}

LnFoldImage pack_ln_fold(const StackedRows &s, const float *gamma, const float *beta, const float *bias) {
    const int64_t K = s.K;
    LnFoldImage f{std::vector<_Float16>((size_t)s.N_pad * K, (_Float16)0), std::vector<_Float16>((size_t)s.N * 16, (_Float16)0)};
    std::vector<_Float16> row((size_t)K);
    s.for_each_row([&](int64_t n, const uint8_t *src) {
        row_to_f16(s.type, K, src, row.data());                          // (the values the un-folded f16 image holds)
        double sum = 0.0, c = bias ? (double)bias[n] : 0.0;
        for (int64_t k = 0; k < K; ++k) {
            const _Float16 wf = (_Float16)((float)row[k] * gamma[k]);
            f.img[(size_t)n * K + k] = wf;
            sum += (double)(float)wf;
            c += (double)beta[k] * (double)(float)row[k];
        }
        const _Float16 s_h = (_Float16)(float)sum, s_l = (_Float16)(float)(sum - (double)(float)s_h);
        const _Float16 c_h = (_Float16)(float)c, c_l = (_Float16)(float)(c - (double)(float)c_h);
        _Float16 *a = f.aug.data() + (size_t)n * 16;
        a[0] = s_h; a[1] = s_l; a[2] = s_h; a[3] = c_h; a[4] = c_l; a[5] = c_h;
    });
    return f;
}

std::vector<uint32_t> pack_gamma_beta_bias(const float *gamma, const float *beta, const float *bias, int64_t n) {
    std::vector<uint32_t> v((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const _Float16 g = (_Float16)gamma[i], bb = (_Float16)(beta[i] + bias[i]);
        uint16_t gu, bu;
        memcpy(&gu, &g, 2); memcpy(&bu, &bb, 2);
        v[(size_t)i] = (uint32_t)gu | ((uint32_t)bu << 16);
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// images on the device
// ------------------------------------------------------------------------------------------------
static bool describe(GemmWeightStore &g, const std::vector<const HostTensor *> &rows, StackedRows &s, std::string &err) {
    if (!s.stack(rows, err)) return false;
    g.w.N = (int)s.N; g.w.K = (int)s.K; g.w.N_pad = (int)s.N_pad;
    g.mfma_ok = s.mfma_ok;
    return true;
}

bool GemmWeightStore::build(const std::vector<const HostTensor *> &rows, const PackOptions &opt, std::string &err) {
    StackedRows s;
    if (!describe(*this, rows, s, err)) return false;
    std::vector<_Float16> img;                                // the rows as f16: the padded image, or naive16's N rows alone
    if (mfma_ok && !(s.q4() && !opt.expand_q4)) {
        // (expand_q4: the values the fused-dequant kernels build in registers on every tile, here once)
        w.type = GW_F16;
        img = pack_f16_image(s, s.N_pad);
        if (!w16.upload(img, err)) return false;
        w.w16 = w16.as<half_t>();
        if (opt.kperm && s.K % 16 == 0) {
            if (!w16p.upload(permute_k16(img), err)) return false;
            w.w16p = w16p.as<half_t>();
        }
    } else if (mfma_ok) {
        w.type = s.type == W_Q4_0 ? GW_Q4_0 : GW_Q4_1;
        const Q4Planes pl = pack_q4_planes(s);
        if (!qs.upload(pl.qs, err) || !sc.upload(pl.sc, err)) return false;
        w.qs = qs.as<uint4>();
        w.sc = sc.p;
    }
    if (opt.naive || !mfma_ok) {
        if (img.empty()) img = pack_f16_image(s, s.N);
        if (!naive16.upload(img.data(), (size_t)s.N * s.K * 2, err)) return false;      // (of the padded image: its first N rows)
        w.naive16 = naive16.as<half_t>();
    }
    if (opt.f32 && s.type == W_F32) {
        std::vector<uint8_t> all;
        for (auto *t : rows) all.insert(all.end(), t->data, t->data + t->nbytes);
        if (all.size() != (size_t)s.N * s.K * 4) { err = "f32 tensor size mismatch"; return false; }
        if (!w32.upload(all, err)) return false;
        w.w32 = w32.as<float>();
    }
    return true;
}

bool GemmWeightStore::build_ln_fold(const std::vector<const HostTensor *> &rows, const float *gamma, const float *beta, const float *bias,
                                    DevBuf &waug, std::string &err) {
    StackedRows s;
    if (!describe(*this, rows, s, err)) return false;
    if (!mfma_ok) return true;                                // (shapes the MFMA kernels do not take are never folded)
    w.type = GW_F16;
    const LnFoldImage f = pack_ln_fold(s, gamma, beta, bias);
    if (!w16.upload(f.img, err) || !waug.upload(f.aug, err)) return false;
    w.w16 = w16.as<half_t>();
    return true;
}

// ------------------------------------------------------------------------------------------------
// ModelWeights
// ------------------------------------------------------------------------------------------------
namespace {

// The tensors of the file by role.  ModelFile::load refuses a file that lacks an expected tensor, holds a 2-D tensor in another
// type than the file-wide one (hp.f16) or a 1-D tensor in another than f32, or disagrees with the hparams in a shape: everything
// below relies on that.  A ModelFile filled by other means gets the one check of resolve().
struct LayerTensors {
    const HostTensor *q, *k, *v, *o, *ffi, *ffo;                                 // [out][in], the file-wide type
    const HostTensor *q_b, *k_b, *v_b, *o_b, *ffi_b, *ffo_b;                     // f32
    const HostTensor *ln_att_w, *ln_att_b, *ln_out_w, *ln_out_b;                 // f32
};
struct ModelTensors {
    const HostTensor *word, *type, *pos, *ln_e_w, *ln_e_b;
    std::vector<LayerTensors> layers;
};

bool resolve(const ModelFile &mf, ModelTensors &m, std::string &err) {
    auto get = [&](const HostTensor *&t, const std::string &name) {
        t = mf.find(name);
        if (!t && err.empty()) err = "tensor '" + name + "' is missing from the model";
    };
    get(m.word, "embeddings.word_embeddings.weight");
    get(m.type, "embeddings.token_type_embeddings.weight");
    get(m.pos, "embeddings.position_embeddings.weight");
    get(m.ln_e_w, "embeddings.LayerNorm.weight");
    get(m.ln_e_b, "embeddings.LayerNorm.bias");
    m.layers.resize(mf.hp.n_layer);
    for (int i = 0; i < mf.hp.n_layer; ++i) {
        const std::string p = "encoder.layer." + std::to_string(i) + ".";
        LayerTensors &l = m.layers[i];
        get(l.q, p + "attention.self.query.weight");        get(l.q_b, p + "attention.self.query.bias");
        get(l.k, p + "attention.self.key.weight");          get(l.k_b, p + "attention.self.key.bias");
        get(l.v, p + "attention.self.value.weight");        get(l.v_b, p + "attention.self.value.bias");
        get(l.o, p + "attention.output.dense.weight");      get(l.o_b, p + "attention.output.dense.bias");
        get(l.ln_att_w, p + "attention.output.LayerNorm.weight");
        get(l.ln_att_b, p + "attention.output.LayerNorm.bias");
        get(l.ffi, p + "intermediate.dense.weight");        get(l.ffi_b, p + "intermediate.dense.bias");
        get(l.ffo, p + "output.dense.weight");              get(l.ffo_b, p + "output.dense.bias");
        get(l.ln_out_w, p + "output.LayerNorm.weight");
        get(l.ln_out_b, p + "output.LayerNorm.bias");
    }
    return err.empty();
}

bool upload_tensor(DevBuf &b, const HostTensor *t, std::string &err) { return b.upload(t->data, t->nbytes, err); }

// 1-D f32 tensors copied out, one after another (their bytes in the file buffer have no alignment guarantee)
std::vector<float> f32_values(std::initializer_list<const HostTensor *> ts) {
    std::vector<float> v;
    for (auto *t : ts) {
        v.resize(v.size() + t->nbytes / 4);
        memcpy(v.data() + v.size() - t->nbytes / 4, t->data, t->nbytes / 4 * 4);
    }
    return v;
}

}  // namespace

bool ModelWeights::naive_images() const {
    for (const LayerWeights &L : layers)
        for (const GemmWeightStore *g : {&L.qkv, &L.o, &L.ffi, &L.ffo})
            if (!g->w.naive16) return false;
    return true;
}

std::unique_ptr<ModelWeights> ModelWeights::load(const ModelFile &mf, const LoadOptions &opt, std::string &err) {
    const HParams &hp = mf.hp;
    const int H = hp.n_embd;
    if (H % 2 != 0) { err = "n_embd must be even"; return nullptr; }
    ModelTensors t;
    if (!resolve(mf, t, err)) return nullptr;
    std::unique_ptr<ModelWeights> w(new ModelWeights);
    const bool q4_file = hp.f16 == W_Q4_0 || hp.f16 == W_Q4_1;
    w->f32_file = hp.f16 == W_F32;

    bool ok = true;
    if (q4_file && opt.expand_q4) {
        w->table_type = W_F32;
        ok = w->word_emb.upload(table_as_f32(*t.word), err) && w->type_emb.upload(table_as_f32(*t.type), err) &&
             w->pos_emb.upload(table_as_f32(*t.pos), err);
    } else {
        w->table_type = hp.f16;
        ok = upload_tensor(w->word_emb, t.word, err) && upload_tensor(w->type_emb, t.type, err) && upload_tensor(w->pos_emb, t.pos, err);
    }
    ok = ok && upload_tensor(w->ln_e_w, t.ln_e_w, err) && upload_tensor(w->ln_e_b, t.ln_e_b, err);

    PackOptions po;
    po.naive = opt.naive; po.expand_q4 = opt.expand_q4; po.f32 = w->f32_file;
    PackOptions po_ffn = po;
    // the k-permuted second image of the FFN weights is only read by layer_tail_kernel (H = 256 / 384)
    po_ffn.kperm = H % 128 == 0 && H >= 256 && H <= 384;
    w->layers = std::vector<LayerWeights>((size_t)hp.n_layer);
    for (int i = 0; ok && i < hp.n_layer; ++i) {
        const LayerTensors &f = t.layers[i];
        LayerWeights &L = w->layers[i];
        ok = L.qkv.build({f.q, f.k, f.v}, po, err);
        // (LayerWeights::qkv_q4: the planes beside an f16 image of more than 3 MiB)
        if (ok && q4_file && opt.expand_q4 && L.qkv.mfma_ok && (size_t)L.qkv.w.N * L.qkv.w.K * 2 > ((size_t)3 << 20))
            ok = L.qkv_q4.build({f.q, f.k, f.v}, PackOptions(), err);
        ok = ok && L.qkv_b.upload(f32_values({f.q_b, f.k_b, f.v_b}), err);
        ok = ok && L.o.build({f.o}, po, err) && upload_tensor(L.o_b, f.o_b, err);
        ok = ok && upload_tensor(L.ln_att_w, f.ln_att_w, err) && upload_tensor(L.ln_att_b, f.ln_att_b, err);
        ok = ok && L.ffi.build({f.ffi}, po_ffn, err) && upload_tensor(L.ffi_b, f.ffi_b, err);
        ok = ok && L.ffo.build({f.ffo}, po_ffn, err) && upload_tensor(L.ffo_b, f.ffo_b, err);
        ok = ok && upload_tensor(L.ln_out_w, f.ln_out_w, err) && upload_tensor(L.ln_out_b, f.ln_out_b, err);
    }
    // LayerNorm folding (kernels.h GemmLnFold; the route of models the fused H <= 384 kernels do not take): images for every layer
    // whose four matrices run on gemm256's f16 form; only when folding is on at load (no option can turn it on without them)
    w->fold_images = opt.ln_fold;
    auto f16_256 = [](const GemmWeightStore &s) { return s.mfma_ok && s.w.type == GW_F16 && s.w.N % 256 == 0 && s.w.K % 64 == 0 && s.w.K >= 128; };
    for (int i = 0; ok && w->fold_images && !w->f32_file && H > 384 && H % 256 == 0 && i < hp.n_layer; ++i) {
        const LayerTensors &f = t.layers[i];
        LayerWeights &L = w->layers[i];
        if (!(f16_256(L.qkv) && f16_256(L.o) && f16_256(L.ffi) && f16_256(L.ffo))) continue;
        const std::vector<float> g1 = f32_values({f.ln_att_w}), b1 = f32_values({f.ln_att_b}), bi = f32_values({f.ffi_b}),
                                 bo2 = f32_values({f.ffo_b});
        ok = L.ffi_fold.build_ln_fold({f.ffi}, g1.data(), b1.data(), bi.data(), L.ffi_waug, err) &&
             L.ffo_gb.upload(pack_gamma_beta_bias(g1.data(), b1.data(), bo2.data(), H), err);
        if (ok && i >= 1) {
            const LayerTensors &prev = t.layers[i - 1];
            const std::vector<float> g2 = f32_values({prev.ln_out_w}), b2 = f32_values({prev.ln_out_b}), bo = f32_values({f.o_b}),
                                     qb = f32_values({f.q_b, f.k_b, f.v_b});
            ok = L.qkv_fold.build_ln_fold({f.q, f.k, f.v}, g2.data(), b2.data(), qb.data(), L.qkv_waug, err) &&
                 L.o_gb.upload(pack_gamma_beta_bias(g2.data(), b2.data(), bo.data(), H), err);
        }
        L.fold_ok = ok && L.ffi_fold.mfma_ok && (i == 0 || L.qkv_fold.mfma_ok);
    }
    // the classification head (ModelFile::load: all four tensors or none, shapes checked)
    if (ok && mf.n_labels > 0) {
        const HostTensor *wp = mf.find("pooler.dense.weight"), *bp = mf.find("pooler.dense.bias"), *wc = mf.find("classifier.weight"),
                         *bc = mf.find("classifier.bias");
        if (!wp || !bp || !wc || !bc) { err = "the classification head is incomplete"; return nullptr; }
        StackedRows s;
        ok = s.stack({wp}, err) && w->head_wp16.upload(pack_f16_image(s, s.N), err) && upload_tensor(w->head_bp, bp, err) &&
             w->head_wc.upload(tensor_as_f32(*wc), err) && upload_tensor(w->head_bc, bc, err);
        if (ok && w->f32_file) ok = upload_tensor(w->head_wp32, wp, err);
        w->n_labels = mf.n_labels;
    }
    // the MLM head (ModelFile::load: all five tensors or none, shapes checked)
    if (ok && mf.mlm_head) {
        const HostTensor *wt = mf.find("cls.predictions.transform.dense.weight"), *bt = mf.find("cls.predictions.transform.dense.bias"),
                         *lw = mf.find("cls.predictions.transform.LayerNorm.weight"), *lb = mf.find("cls.predictions.transform.LayerNorm.bias"),
                         *bv = mf.find("cls.predictions.bias");
        if (!wt || !bt || !lw || !lb || !bv) { err = "the MLM head is incomplete"; return nullptr; }
        ok = w->mlm_wt.build({wt}, po, err) && upload_tensor(w->mlm_bt, bt, err) && upload_tensor(w->mlm_ln_w, lw, err) &&
             upload_tensor(w->mlm_ln_b, lb, err) && upload_tensor(w->mlm_bias, bv, err);
        if (ok && hp.f16 == W_F16) w->vocab16 = w->word_emb.as<half_t>();
        else if (ok) {
            StackedRows s;
            ok = s.stack({t.word}, err) && w->vocab16_own.upload(pack_f16_image(s, s.N), err);
            w->vocab16 = w->vocab16_own.as<half_t>();
        }
        w->mlm_head = ok;
    }
    // the relative position bias (ModelFile::load: [REL_BUCKETS][n_head], f32 or f16)
    if (ok && mf.rel_bias) {
        const HostTensor *rb = mf.find(REL_BIAS_NAME);
        if (!rb) { err = "the relative position bias is missing"; return nullptr; }
        const std::vector<float> W = tensor_as_f32(*rb);
        ok = w->rel.upload(rel_bias_table(W.data(), hp.n_head, hp.n_max_tokens, 1.0), err) &&
             w->rel_scaled.upload(rel_bias_table(W.data(), hp.n_head, hp.n_max_tokens, std::sqrt((double)(H / hp.n_head))), err);
        w->rel_bias = ok;
    }
    if (!ok) return nullptr;
    return w;
}

}  // namespace bert_hip
