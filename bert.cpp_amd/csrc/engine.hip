// engine.hip — see engine.h.
#include "engine.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <system_error>
#include <thread>

namespace bert_hip {

Engine *Engine::create(const ModelFile &mf, int device, std::string &err) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        err = "no HIP device available (this library needs an AMD GPU; there is no CPU fallback)";
        return nullptr;
    }
    if (device < 0 || device >= ndev) { err = "HIP device ordinal " + std::to_string(device) + " out of range"; return nullptr; }
    std::unique_ptr<Engine> e(new Engine);
    e->hp_ = mf.hp;
    e->device_ = device;
    if (hipSetDevice(e->device_) != hipSuccess) { err = "hipSetDevice failed"; return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e->device_) != hipSuccess) { err = "hipGetDeviceProperties failed"; return nullptr; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        err = std::string("unsupported GPU architecture '") + prop.gcnArchName + "' (kernels are built for gfx950 / MI355X only)";
        return nullptr;
    }
    e->opt_ = EngineOptions::from_env(mf.hp);
    LoadOptions lo;
    lo.naive = e->opt_.gemm_naive; lo.expand_q4 = e->opt_.q4_expand; lo.ln_fold = e->opt_.ln_fold;
    e->w_ = ModelWeights::load(mf, lo, err);
    if (!e->w_ || !e->status_.alloc(16, err)) return nullptr;
    if (hipStreamCreateWithFlags(&e->stream_, hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; return nullptr; }
    if (hipEventCreateWithFlags(&e->busy_, hipEventDisableTiming) != hipSuccess) { err = "hipEventCreate failed"; return nullptr; }
    return e.release();
}

Engine::~Engine() {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    for (auto &sl : slot_) {
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (busy_) (void)hipEventDestroy(busy_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

bool Engine::reserve(int n_tokens, int n_sentences, std::string &err) {
    HIP_OK(hipSetDevice(device_), err, false);
    if (n_tokens <= 0 || n_sentences <= 0) return true;
    return ensure_workspace((n_tokens + 255) / 256 * 256, n_sentences, err) && (!w_->mlm_head || ensure_sparse(n_sentences, err));
}

int Engine::check(std::string &err) {
    HIP_OK(hipSetDevice(device_), err, -1);
    HIP_OK(hipDeviceSynchronize(), err, -1);
    int st = 0;
    HIP_OK(hipMemcpy(&st, status_.p, sizeof(int), hipMemcpyDeviceToHost), err, -1);
    if (st) HIP_OK(hipMemset(status_.p, 0, sizeof(int)), err, -1);
    return st;
}

void Engine::set_option(const std::string &key, const std::string &value) {
    if (key == "profile_replay") { prof_.set_replay(value); return; }
    (void)hipSetDevice(device_);
    if (!test_poison_option(key, ctx_, y_, {&x_, &qkv_, &ctx_, &y_, &ff_, &v32_, &ln_stats1_, &ln_stats2_, &ln_rows1_, &ln_rows2_, &d_hidden_})) opt_.set(key, value, w_->naive_images(), w_->fold_images);
}

bool Engine::ensure_workspace(int t_pad, int n_sentences, std::string &err) {
    const size_t H = hp_.n_embd, I = hp_.n_intermediate, tp = (size_t)t_pad;
    const size_t es = w_->f32_file ? 4 : 2;                      // (f32 files: the f32 route's activations are f32)
    return x_.ensure(tp * H * es, err) && qkv_.ensure(tp * 3 * H * es, err) && ctx_.ensure(tp * H * es, err) &&
           y_.ensure(tp * H * es, err) && ff_.ensure(tp * I * es, err) && v32_.ensure((size_t)std::max(128, std::min(t_pad, (opt_.latency_tokens + 255) / 256 * 256)) * H * 4, err) &&
           d_out_.ensure((size_t)n_sentences * H * 4, err) &&
           windows_.ensure((size_t)n_sentences * sizeof(int2), err) &&
           // (LayerNorm folding, H = 768 route: 2 H / 256 partial (sum, sum of squares) pairs and one finalized float4 per row and LayerNorm)
           (!(H > 384 && H % 256 == 0) || (ln_stats1_.ensure(tp * (2 * H / 256) * 8, err) && ln_stats2_.ensure(tp * (2 * H / 256) * 8, err) &&
                                           ln_rows1_.ensure(tp * 16, err) && ln_rows2_.ensure(tp * 16, err)));
}

void Engine::timed_launch(const char *name, double flops, hipStream_t s, const std::function<void()> &f) { timed(name, flops, s, f); }

bool Engine::op_begin(hipStream_t s, hipEvent_t busy, StreamOp &op, std::string &err) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    HIP_OK(hipStreamIsCapturing(s, &st), err, false);
    // (only an ACTIVE capture.  A stream whose capture was invalidated — by an allocation, say — takes the eager path: the runtime
    // refuses the wait or the launches on it itself, and goes on doing so after hipStreamEndCapture: such a stream is to be destroyed)
    op.s = s; op.busy = busy; op.capturing = st == hipStreamCaptureStatusActive;
    if (!op.capturing) {
        if (busy) HIP_OK(hipStreamWaitEvent(s, busy, 0), err, false);
        return true;
    }
    if (prof_.enabled()) { err = "the stream is capturing while the context profiles: a timed launch cannot be captured (bert_hip_profile_enable(ctx, 0) first)"; return false; }
    return true;
}

bool Engine::op_end(const StreamOp &op, std::string &err) {
    if (!op.capturing && op.busy) HIP_OK(hipEventRecord(op.busy, op.s), err, false);
    return true;
}

std::string Engine::profile_report() {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    return prof_.report();
}

void Engine::build_windows(const int32_t *cu, int B, std::vector<int2> &windows, int slot) {
    windows.clear();                                          // slot: 16 (or 8: kernels.h), the value the pass read once
    int first = 0, fill = 0;                                  // open window: sentences first .. b-1 occupy `fill` slots
    for (int b = 0; b < B; ++b) {
        const int n = cu[b + 1] - cu[b];
        if (b > first && fill + n > 128) {
            windows.push_back(make_int2(first, b - first));
            first = b; fill = 0;
        }
        fill = (fill + n + slot - 1) & ~(slot - 1);
    }
    if (B > first) windows.push_back(make_int2(first, B - first));
}

int Engine::eval_packed_device(const int32_t *d_tokens, const int32_t *d_cu, int B, int T, int max_len, float *d_out,
                               hipStream_t s, float *d_hidden, std::string &err, const int2 *d_windows, int n_windows, int slots_in,
                               int pool_mode_in, void *d_token_rows, int token_flags, const int32_t *d_first_len) {
    if (B <= 0 || T <= 0) return 0;
    // the windows' place granularity, read ONCE per pass (the host path read it when it built its list): the window list, the
    // grid bound and the kernels' place rule must agree whatever another thread or context sets meanwhile
    const int slots = slots_in ? slots_in : window_slots();
    // (so are "pooling" and "normalize": every launch that ends the pass gets the plan's value)
    const int pool_mode = pool_mode_in >= 0 ? pool_mode_in : opt_.pool_mode();
    HIP_OK(hipSetDevice(device_), err, -1);
    // one forward pass at a time on the shared workspace: wait (on the caller's stream) for the previous pass — unless s is capturing
    StreamOp op;
    if (!op_begin(s, busy_, op, err)) return -1;
    if (!ensure_workspace((T + 255) / 256 * 256, B, err)) return -1;
    prof_.begin_pass();
    if (!d_out) d_out = d_out_.as<float>();                   // (a token-rows call that wants no embeddings: ensure_workspace sized it)
    const Plan p = plan(d_tokens, d_cu, B, T, max_len, d_out, s, d_hidden, d_windows, n_windows, slots, pool_mode, d_token_rows, d_first_len);
    bool ok = true;
    if (p.route == Route::F32) ok = forward_f32(p, err);
    else {
        const int H = hp_.n_embd;
        // (the one-launch kernel's full form: the same values in lane order in y_, no rows — plan() asked the launcher's own rule)
        if (p.embed_lanes)
            timed("embed_ln", 0.0, s, [&] { ok = launch_embed_ln_lanes(w_->word_emb.p, w_->type_emb.p, w_->pos_emb.p, w_->table_type, w_->ln_e_w.as<float>(), w_->ln_e_b.as<float>(),
                                                                       d_tokens, d_cu, B, T, H, hp_.n_vocab, max_len, y_.as<half_t>(), s, d_first_len); });
        else
            timed("embed_ln", 0.0, s, [&] { launch_embed_ln(w_->word_emb.p, w_->type_emb.p, w_->pos_emb.p, w_->table_type, w_->ln_e_w.as<float>(), w_->ln_e_b.as<float>(),
                                                            d_tokens, d_cu, B, T, H, hp_.n_vocab, max_len, x_.as<half_t>(), s, d_first_len); });
        if (!ok) { err = "embed_ln: no lane-order kernel for this shape"; return -1; }
        tap(p, 0);
        if (p.build_windows)
            timed("build_windows", 0.0, s, [&] { launch_build_windows(d_cu, B, windows_.as<int2>(), status_.as<int>() + 1, slots, s); });
        switch (p.route) {
            case Route::LATENCY: forward_latency(p); break;
            case Route::ONE_LAUNCH: forward_one_launch(p); break;
            case Route::FOLDED: ok = forward_folded(p, err); break;
            default: ok = forward_layers(p, err); break;
        }
        // (the one-launch kernel's workgroups pool their sentences themselves)
        if (ok && p.route != Route::ONE_LAUNCH)
            timed("pool_normalize", 2.0 * T * H, s, [&] { launch_pool_normalize(x_.as<half_t>(), d_cu, B, H, max_len, status_.as<int>(), d_out, p.pool_mode, s); });
    }
    if (!ok) return -1;
    // (every route a token-rows pass can take left the final states in x_, [T][H] in row order: f32 on the f32 route, else f16)
    // (a destination that IS x_: the caller wants them where they are — the sparse head —, nothing to copy)
    if (d_token_rows && d_token_rows != x_.p)
        timed("token_rows", 0.0, s, [&] { launch_token_rows(x_.p, p.route == Route::F32, T, hp_.n_embd, d_cu, B, max_len, token_flags, d_token_rows, s); });
    HIP_OK(hipGetLastError(), err, -1);
    return op_end(op, err) ? 0 : -1;
}

// The route of a pass and, per layer, its kernels: every eligibility test of the forward pass, each made here once.  Launches nothing.
Engine::Plan Engine::plan(const int32_t *d_tokens, const int32_t *d_cu, int B, int T, int max_len, float *d_out, hipStream_t s,
                          float *d_hidden, const int2 *d_windows, int n_windows, int slots, int pool_mode, void *d_token_rows,
                          const int32_t *d_first_len) const {
    // (t_pad: whole tiles of every kernel family, 128- and 256-token tiles)
    Plan p{d_tokens, d_cu, B, T, max_len, (T + 255) / 256 * 256, slots, pool_mode, d_out, d_hidden, d_token_rows, d_first_len, s, d_windows, n_windows};
    if (w_->f32_file && opt_.f32_exact) { p.route = Route::F32; return p; }
    const int H = hp_.n_embd, nh = hp_.n_head, dh = H / nh, Lz = hp_.n_layer;
    auto family = [&](const GemmWeightStore &W) {
        if (W.mfma_ok && opt_.gemm256 && !opt_.gemm_naive && gemm256_supported(W.w, p.t_pad)) return Family::GEMM256;
        return W.mfma_ok && (!opt_.gemm_naive || !W.w.naive16) ? Family::MFMA : Family::NAIVE;
    };
    // per layer (a file may mix types or shapes from layer to layer): its stages and mat-mul kernels, and whether it can run in the
    // one-launch kernel (which takes all layers' pointers) or with its LayerNorms folded (only models the fused kernels do not take)
    p.layers.resize(Lz);
    bool qkv2_shape0 = false, one_launch = true, fold = opt_.ln_fold && H > 384 && H % 256 == 0 && ln_rows2_.p;
    // a relative position bias (MPNet files) lives in the attention launch alone: such a model takes none of the kernels that hold an
    // attention of their own — qkv_attention2, and with it the one-launch kernel, and the latency route, which shares their bits
    const bool fused_attention = !w_->rel_bias;
    for (int il = 0; il < Lz; ++il) {
        const LayerWeights &L = w_->layers[il];
        LayerPlan &lp = p.layers[il];
        const bool qkv2_shape = qkv_attention2_supported(L.qkv.w, nh, dh, max_len), tail_shape = layer_tail_supported(L.o.w, L.ffi.w, L.ffo.w);
        if (il == 0) qkv2_shape0 = qkv2_shape;
        lp.qkv2 = fused_attention && opt_.qkv2 && !opt_.gemm_naive && !opt_.attn_naive && L.qkv.mfma_ok && qkv2_shape;
        lp.tail = opt_.tail && !opt_.gemm_naive && L.o.mfma_ok && L.ffi.mfma_ok && L.ffo.mfma_ok && tail_shape;
        // (q4 files: the 4-bit planes of the stacked matrix where its f16 image overflows an XCD's L2 and gemm256 takes the launch)
        lp.planes = L.qkv_q4.w.qs && family(L.qkv_q4) == Family::GEMM256;
        lp.qkv = family(lp.planes ? L.qkv_q4 : L.qkv), lp.o = family(L.o), lp.ffi = family(L.ffi), lp.ffo = family(L.ffo);
        one_launch = one_launch && L.qkv.mfma_ok && L.o.mfma_ok && L.ffi.mfma_ok && L.ffo.mfma_ok && L.ffi.w.w16p && L.ffo.w.w16p &&
                     model_kernel_supported(L.qkv.w, L.o.w, L.ffi.w, L.ffo.w, Lz, nh, dh, max_len);
        fold = fold && L.fold_ok && (il ? family(L.qkv_fold) : lp.qkv) == Family::GEMM256 && lp.o == Family::GEMM256 &&
               family(L.ffi_fold) == Family::GEMM256 && lp.ffo == Family::GEMM256 && !(opt_.qkv2 && qkv2_shape) && !(opt_.tail && tail_shape);
    }
    // a hidden-state tap wants every layer's normalised states: it takes neither the one-launch kernel nor the folded LayerNorms
    if (d_hidden) one_launch = fold = false;
    // token rows want the last layer's states in x_ in row order: not the one-launch kernel; the folded LayerNorms stay
    if (d_token_rows) one_launch = false;
    const bool fused_windows = p.layers[0].qkv2, latency_call = opt_.latency && T <= opt_.latency_tokens;
    one_launch = one_launch && fused_windows && opt_.one_launch && opt_.tail && !latency_call;
    // sentence windows of the fused projection+attention kernel: the caller's (host path), or built on the device from cu_seqlens
    // when packing can pay — sentences on average clearly shorter than max_len; for full-length batches the uniform rule
    // (max_len-sized places) gives the same windows without the extra launch.  (Forced one-launch: the kernel takes a window list
    // or one sentence per window — its layer-tail phase needs a window's tokens to be at most 128 whatever the sentences' lengths.)
    const bool full_windows = (long long)B * 128 == T;
    // (the one-launch kernel's full form starts from the embedding in lane order and reads no rows: a batch of that shape whose tables the
    // lane-order embedding kernel does not take leaves the route)
    if (full_windows && !embed_ln_lanes_supported(w_->table_type, H, T, max_len)) one_launch = false;
    const int spw = qkv_attention2_sentences_per_window(max_len, slots);
    if (!d_windows && fused_windows &&
        (4ll * ((B + spw - 1) / spw) * 128 > 5 * ((long long)T + (long long)(slots / 2) * B) || (one_launch && opt_.one_launch == 2 && spw > 1 && !full_windows))) {
        p.build_windows = true;
        p.windows = windows_.as<int2>();
        p.n_windows_dev = status_.as<int>() + 1;
        // upper bound from T and B alone (the extra workgroups return at once): "never more than the uniform rule" only holds for
        // batches that keep their max_len promise, and a broken promise must cost the offender its row, not a neighbour its window
        p.n_windows = qkv_attention2_max_windows(B, T, slots);
    }
    // When the one-launch kernel pays: its layer-tail phase costs a window 128 rows' time however few tokens it holds, the layer-tail
    // KERNEL runs on the packed tokens — 0.32 + 0.68 fill against 0.94 (full windows: +6.7 %): from a fill of 0.91.  The window
    // count is known for the caller's list and for one sentence per window, not for a list built on the device.
    bool one_launch_pays = full_windows || opt_.one_launch == 2;
    if (!one_launch_pays && !p.build_windows) one_launch_pays = (d_windows || spw == 1) && 100ll * T >= 95ll * 128 * (d_windows ? n_windows : B);
    const LayerWeights &L0 = w_->layers[0];
    const bool skinny = fused_attention && latency_call && opt_.tail && opt_.qkv2 && !opt_.gemm_naive && !opt_.attn_naive && max_len <= 128 && (dh == 32 || dh == 64) &&
                        skinny_layer_supported(L0.qkv.w, L0.o.w, L0.ffi.w, L0.ffo.w) && qkv2_shape0;
    p.route = skinny ? Route::LATENCY : one_launch && one_launch_pays ? Route::ONE_LAUNCH : fold ? Route::FOLDED : Route::LAYERED;
    // (launch_model_kernel takes its full form by the same rule; neither a tap nor token rows reach this route, nothing else reads x_ on it
    // before the kernel's last layer has written it)
    p.embed_lanes = p.route == Route::ONE_LAUNCH && full_windows;
    return p;
}

// one weight mat-mul on the kernel family the plan chose: counted for the profile ("family:<kernel>_<weights>"), timed, launched.  A
// LayerNorm-folding form that no kernel runs fails the pass (it must not run as the plain mat-mul).
bool Engine::gemm(const Plan &p, const char *name, Family f, const GemmWeightStore &W, const void *A, const float *bias, const void *resid,
                  void *C, int epi, std::string &err, const GemmLnFold *ln) {
    static const char *const kernel[] = {"gemm256", "gemm_mfma", "gemm_naive", "gemm_f32"};
    prof_.count_family(std::string("family:") + kernel[(int)f] + (f == Family::GEMM256 || f == Family::MFMA ? (W.w.type == GW_F16 ? "_f16" : "_q4") : ""));
    const half_t *a = (const half_t *)A, *r = (const half_t *)resid;
    bool ok = !(ln && ln->flags) || f == Family::GEMM256;
    if (ok)
        timed(name, 2.0 * p.T * W.w.N * W.w.K, p.s, [&] {
            if (f == Family::F32) launch_f32_gemm((const float *)A, W.w.w32, bias, (const float *)resid, (float *)C, p.T, W.w.N, W.w.K, epi, p.s);
            else if (f == Family::GEMM256) ok = launch_gemm256(W.w, a, bias, r, (half_t *)C, p.t_pad, epi, p.s, ln);
            else if (f == Family::MFMA) launch_gemm_mfma(W.w, a, bias, r, (half_t *)C, p.t_pad, epi, p.s);
            else launch_gemm_naive(W.w, a, bias, r, (half_t *)C, p.T, epi, p.s);
        });
    if (!ok) err = std::string(name) + ": no " + kernel[(int)f] + " kernel for LayerNorm-folding flags " + std::to_string(ln->flags) + ", epilogue " + std::to_string(epi);
    return ok;
}

// (attention FLOPs: 4 * sum_b N_b^2 * H; only T and max_len are known here -> upper bound T * max_len)
void Engine::attention(const Plan &p) {
    const int H = hp_.n_embd, nh = hp_.n_head, dh = H / nh;
    half_t *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>();
    // (the relative position bias of the file, if it has one: null pointers otherwise)
    const int P = hp_.n_max_tokens;
    timed("attention", 4.0 * p.T * p.max_len * H, p.s, [&] {
        if (opt_.attn_naive || !launch_attention_mfma(qkv, p.cu, p.B, nh, dh, p.max_len, ctx, p.s, w_->rel_scaled.as<float>(), P))
            launch_attention_naive(qkv, p.cu, p.B, nh, dh, p.max_len, ctx, p.s, w_->rel.as<float>(), P);
    });
}

// the layer states of eval_hidden as f32: x after the embedding LayerNorm (idx 0) and after every layer
void Engine::tap(const Plan &p, int idx) {
    const size_t n = (size_t)p.T * hp_.n_embd;
    if (p.hidden && p.route == Route::F32) (void)hipMemcpyAsync(p.hidden + idx * n, x_.p, n * 4, hipMemcpyDeviceToDevice, p.s);
    else if (p.hidden) launch_f16_to_f32(x_.as<half_t>(), p.hidden + idx * n, n, p.s);
}

// The latency route (skinny.hip): a call of a few windows would keep as many CUs of 256 busy on the fused kernels.  Same bits per
// sentence (the route must not show in the results), seven short launches per layer.
void Engine::forward_latency(const Plan &p) {
    const int H = hp_.n_embd, I = hp_.n_intermediate, tb = (p.T + 31) / 32, Lz = hp_.n_layer;
    half_t *x = x_.as<half_t>(), *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>(), *y = y_.as<half_t>(), *ff = ff_.as<half_t>();
    float *v32 = v32_.as<float>();
    for (int il = 0; il < Lz; ++il) {
        const LayerWeights &L = w_->layers[il];
        // (from the second layer on the QKV kernel LayerNorms the previous layer's output itself and writes x)
        const LayerWeights *P = il ? &w_->layers[il - 1] : nullptr;
        timed("skinny_qkv", 2.0 * p.T * 3 * H * H, p.s, [&] {
            launch_skinny_gemm(0, L.qkv.w, x, P ? v32 : nullptr, P ? P->ln_out_w.as<float>() : nullptr, P ? P->ln_out_b.as<float>() : nullptr,
                               x, L.qkv_b.as<float>(), nullptr, qkv, nullptr, tb, p.s);
        });
        attention(p);
        timed("skinny_proj", 2.0 * p.T * H * H, p.s, [&] {
            launch_skinny_gemm(1, L.o.w, ctx, nullptr, nullptr, nullptr, nullptr, L.o_b.as<float>(), x, nullptr, v32, tb, p.s);
        });
        timed("skinny_ffn_up", 2.0 * p.T * H * I, p.s, [&] {
            launch_skinny_gemm(2, L.ffi.w, nullptr, v32, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), y, L.ffi_b.as<float>(), nullptr, ff, nullptr, tb, p.s);
        });
        timed("skinny_ffn_down", 2.0 * p.T * H * I, p.s, [&] {
            launch_skinny_gemm(3, L.ffo.w, ff, nullptr, nullptr, nullptr, nullptr, L.ffo_b.as<float>(), y, nullptr, v32, tb, p.s);
        });
        // (the last layer, or a hidden-state tap: somebody has to materialise x now; the next QKV kernel writes the same bits again)
        if (il + 1 == Lz || p.hidden)
            timed("skinny_layernorm", 0.0, p.s, [&] { launch_skinny_layernorm(v32, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), x, tb, H, p.s); });
        tap(p, il + 1);
    }
}

// All layers in one launch, a workgroup per window (model_kernel.hip) — the two fused kernels' bodies as phases, no kernel boundary
// to put the workgroups back in step.  Batches of FULL windows (every sentence exactly 128 tokens: T = 128 B) take the specialised
// form (every window is one whole sentence, whatever list the caller built); between its layers the residual crosses in lane order through
// the y workspace, which this route uses for nothing else (not through ctx: the full form must not touch that one at all).
void Engine::forward_one_launch(const Plan &p) {
    const int H = hp_.n_embd, I = hp_.n_intermediate;
    ModelLayerWeights mw[MODEL_MAX_LAYERS];          // (plan(): model_kernel_supported refuses more layers)
    for (int il = 0; il < hp_.n_layer; ++il) {
        const LayerWeights &L = w_->layers[il];
        mw[il] = {&L.qkv.w, &L.o.w, &L.ffi.w, &L.ffo.w, L.qkv_b.as<float>(), L.o_b.as<float>(), L.ln_att_w.as<float>(), L.ln_att_b.as<float>(),
                  L.ffi_b.as<float>(), L.ffo_b.as<float>(), L.ln_out_w.as<float>(), L.ln_out_b.as<float>()};
    }
    timed("model_kernel", hp_.n_layer * (2.0 * p.T * 3 * H * H + 4.0 * p.T * p.max_len * H + 2.0 * p.T * H * H + 4.0 * p.T * H * I), p.s, [&] {
        launch_model_kernel(mw, hp_.n_layer, x_.as<half_t>(), ctx_.as<half_t>(), y_.as<half_t>(), p.cu, p.B, p.T, p.windows, p.n_windows, p.n_windows_dev, hp_.n_head,
                            p.out, p.max_len, status_.as<int>(), p.pool_mode, p.slots, p.s);
    });
}

// LayerNorm folding (kernels.h GemmLnFold; the plan put every mat-mul on gemm256's f16 form): the layers keep the UN-normalised sums
// u1 (in y) and u2 (in x) and never launch a LayerNorm of their own but the last one
bool Engine::forward_folded(const Plan &p, std::string &err) {
    const int H = hp_.n_embd, P = 2 * H / 256;
    const Family G = Family::GEMM256;
    half_t *x = x_.as<half_t>(), *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>(), *y = y_.as<half_t>(), *ff = ff_.as<half_t>();
    float2 *st1 = ln_stats1_.as<float2>(), *st2 = ln_stats2_.as<float2>();
    float4 *rows1 = ln_rows1_.as<float4>(), *rows2 = ln_rows2_.as<float4>();
    for (int il = 0; il < hp_.n_layer; ++il) {
        const LayerWeights &L = w_->layers[il];
        GemmLnFold ln;
        if (il == 0) {
            // x = LayerNorm(embeddings), materialised by the embedding kernel: the plain projection (4-bit planes where the file has them)
            if (!gemm(p, "gemm_qkv", G, p.layers[0].planes ? L.qkv_q4 : L.qkv, x, L.qkv_b.as<float>(), nullptr, qkv, EPI_BIAS, err)) return false;
        } else {
            // x holds u2 of the layer before: its output LayerNorm rides in the folded weights, the statistics k-step and the row scale
            ln.flags = GemmLnFold::IN; ln.rows_in = rows2; ln.waug = L.qkv_waug.as<half_t>();
            if (!gemm(p, "gemm_qkv", G, L.qkv_fold, x, nullptr, nullptr, qkv, EPI_BIAS, err, &ln)) return false;
        }
        attention(p);
        // u1 = ctx Wo^T + bo + (x | LayerNorm(u2 of the layer before)) -> y, with its rows' partial statistics
        ln = GemmLnFold(); ln.flags = GemmLnFold::STATS | (il ? GemmLnFold::RES : 0); ln.stats = st1; ln.rows_res = rows2; ln.gb = L.o_gb.as<unsigned>();
        if (!gemm(p, "gemm_attn_out", G, L.o, ctx, L.o_b.as<float>(), x, y, EPI_BIAS_RESID, err, &ln)) return false;
        timed("ln_rows_finalize", 0.0, p.s, [&] { launch_ln_rows_finalize(st1, P, p.t_pad, H, rows1, p.s); });
        ln = GemmLnFold(); ln.flags = GemmLnFold::IN; ln.rows_in = rows1; ln.waug = L.ffi_waug.as<half_t>();
        if (!gemm(p, "gemm_ffn_up", G, L.ffi_fold, y, nullptr, nullptr, ff, EPI_BIAS_GELU, err, &ln)) return false;
        // u2 = ff W2^T + b2 + LayerNorm(u1) -> x
        ln = GemmLnFold(); ln.flags = GemmLnFold::STATS | GemmLnFold::RES; ln.stats = st2; ln.rows_res = rows1; ln.gb = L.ffo_gb.as<unsigned>();
        if (!gemm(p, "gemm_ffn_down", G, L.ffo, ff, L.ffo_b.as<float>(), y, x, EPI_BIAS_RESID, err, &ln)) return false;
        timed("ln_rows_finalize", 0.0, p.s, [&] { launch_ln_rows_finalize(st2, P, p.t_pad, H, rows2, p.s); });
        if (il + 1 == hp_.n_layer)     // (the pooling reads normalised rows: the one LayerNorm launch of the pass)
            timed("layernorm", 0.0, p.s, [&] { launch_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.T, H, p.s); });
    }
    return true;
}

// A layer at a time, each with the stages and mat-mul kernels the plan chose for it
bool Engine::forward_layers(const Plan &p, std::string &err) {
    const int H = hp_.n_embd, I = hp_.n_intermediate;
    half_t *x = x_.as<half_t>(), *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>(), *y = y_.as<half_t>(), *ff = ff_.as<half_t>();
    for (int il = 0; il < hp_.n_layer; ++il) {
        const LayerWeights &L = w_->layers[il];
        const LayerPlan &lp = p.layers[il];
        if (lp.qkv2) {
            // windows of 128 token slots holding whole sentences: Q|K|V never reach HBM whatever the sentence lengths
            timed("qkv_attention2", 2.0 * p.T * L.qkv.w.N * L.qkv.w.K + 4.0 * p.T * p.max_len * H, p.s, [&] {
                launch_qkv_attention2(L.qkv.w, x, L.qkv_b.as<float>(), p.cu, p.B, p.windows, p.n_windows, p.n_windows_dev, p.max_len, hp_.n_head, p.slots, ctx, p.s);
            });
        } else {
            if (!gemm(p, "gemm_qkv", lp.qkv, lp.planes ? L.qkv_q4 : L.qkv, x, L.qkv_b.as<float>(), nullptr, qkv, EPI_BIAS, err)) return false;
            attention(p);
        }
        if (lp.tail) {
            // out-projection + LN + FFN + LN in one launch, a pair of specialist waves per 32 tokens: y and the intermediate never leave the chip
            timed("layer_tail", 2.0 * p.T * H * H + 4.0 * p.T * H * I, p.s, [&] {
                launch_layer_tail(L.o.w, L.ffi.w, L.ffo.w, ctx, x, L.o_b.as<float>(), L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), L.ffi_b.as<float>(),
                                  L.ffo_b.as<float>(), L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), x, p.t_pad, p.s);
            });
        } else {
            if (!gemm(p, "gemm_attn_out", lp.o, L.o, ctx, L.o_b.as<float>(), x, y, EPI_BIAS_RESID, err)) return false;
            timed("layernorm", 0.0, p.s, [&] { launch_layernorm(y, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), p.T, H, p.s); });
            if (!gemm(p, "gemm_ffn_up", lp.ffi, L.ffi, y, L.ffi_b.as<float>(), nullptr, ff, EPI_BIAS_GELU, err) ||
                !gemm(p, "gemm_ffn_down", lp.ffo, L.ffo, ff, L.ffo_b.as<float>(), y, x, EPI_BIAS_RESID, err)) return false;
            timed("layernorm", 0.0, p.s, [&] { launch_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.T, H, p.s); });
        }
        tap(p, il + 1);
    }
    return true;
}

// f32 files at the reference's precision (f32_route.hip; reference bert.cpp:784-913 with GGML_TYPE_F32 tensors): the same
// sequence of operations as the tiled family, every one in f32, with embedding and pooling kernels of its own.
bool Engine::forward_f32(const Plan &p, std::string &err) {
    const int H = hp_.n_embd, nh = hp_.n_head, dh = H / nh;
    const Family F = Family::F32;
    float *x = x_.as<float>(), *qkv = qkv_.as<float>(), *ctx = ctx_.as<float>(), *y = y_.as<float>(), *ff = ff_.as<float>();
    timed("embed_ln", 0.0, p.s, [&] {
        launch_f32_embed_ln(w_->word_emb.as<float>(), w_->type_emb.as<float>(), w_->pos_emb.as<float>(), w_->ln_e_w.as<float>(), w_->ln_e_b.as<float>(), p.tokens,
                            p.cu, p.B, p.T, H, hp_.n_vocab, p.max_len, x, p.s, p.first_len);
    });
    tap(p, 0);
    for (int il = 0; il < hp_.n_layer; ++il) {
        const LayerWeights &L = w_->layers[il];
        if (!gemm(p, "gemm_qkv", F, L.qkv, x, L.qkv_b.as<float>(), nullptr, qkv, EPI_BIAS, err)) return false;
        bool launched = true;
        timed("attention", 4.0 * p.T * p.max_len * H, p.s, [&] { launched = launch_f32_attention(qkv, p.cu, p.B, nh, dh, p.max_len, ctx, p.s, w_->rel.as<float>(), hp_.n_max_tokens); });
        if (!launched) {
            err = "f32 route: the attention kernel keeps the scores of max_len = " + std::to_string(p.max_len) + " keys per wave in LDS, " +
                  std::to_string(f32_attention_lds_bytes(p.max_len)) + " bytes a workgroup; this device's limit is " +
                  std::to_string(f32_attention_lds_limit()) + " bytes (set_option \"f32\" = \"f16\" selects the f16 kernels)";
            return false;
        }
        if (!gemm(p, "gemm_attn_out", F, L.o, ctx, L.o_b.as<float>(), x, y, EPI_BIAS_RESID, err)) return false;
        timed("layernorm", 0.0, p.s, [&] { launch_f32_layernorm(y, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), p.T, H, p.s); });
        if (!gemm(p, "gemm_ffn_up", F, L.ffi, y, L.ffi_b.as<float>(), nullptr, ff, EPI_BIAS_GELU, err) ||
            !gemm(p, "gemm_ffn_down", F, L.ffo, ff, L.ffo_b.as<float>(), y, x, EPI_BIAS_RESID, err)) return false;
        timed("layernorm", 0.0, p.s, [&] { launch_f32_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.T, H, p.s); });
        tap(p, il + 1);
    }
    timed("pool_normalize", 2.0 * p.T * H, p.s, [&] { launch_f32_pool_normalize(x, p.cu, p.B, H, p.max_len, status_.as<int>(), p.out, p.pool_mode, p.s); });
    return true;
}

static bool ensure_pinned(void **p, size_t *cap, size_t need, std::string &err) {
    if (need <= *cap) return true;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    need += need / 4;
    HIP_OK(hipHostMalloc(p, need, hipHostMallocDefault), err, false);
    *cap = need;
    return true;
}

// The rows of a call's LAST chunk leave the pinned block with nothing to hide the copy behind (earlier chunks are copied out under
// the next one's forward pass): a large block goes out on four threads (one core moves ~10 GB/s: 0.9 ms for the 9 MB of 6000
// MiniLM rows).  A thread that cannot be started is not an error: the caller copies its part.
static void copy_rows_out(float *dst, const float *src, size_t bytes) {
    constexpr size_t PART_MIN = (size_t)1 << 20;
    constexpr int MAX_PARTS = 4;
    const int parts = (int)std::min<size_t>(MAX_PARTS, bytes / PART_MIN);
    if (parts <= 1) { memcpy(dst, src, bytes); return; }
    const size_t each = (bytes / parts + 4095) & ~(size_t)4095;
    std::thread helpers[MAX_PARTS - 1];
    size_t inline_from = each;                         // [0, each) is the caller's; [inline_from, bytes) too when a start fails
    for (int k = 1; k < parts; ++k) {
        const size_t off = (size_t)k * each, n = std::min(each, bytes - std::min(bytes, off));
        if (n == 0) break;
        try {
            helpers[k - 1] = std::thread([=] { memcpy((char *)dst + off, (const char *)src + off, n); });
            inline_from = off + n;
        } catch (const std::system_error &) {
            break;
        }
    }
    memcpy(dst, src, std::min(each, bytes));
    if (inline_from < bytes) memcpy((char *)dst + inline_from, (const char *)src + inline_from, bytes - inline_from);
    for (auto &h : helpers)
        if (h.joinable()) h.join();
}

int Engine::eval_packed_host(const int32_t *tokens, const int32_t *cu, int B, float *embeddings, std::string &err,
                             float *d_embeddings, int pool_mode_in) {
    if (B <= 0) return 0;
#ifdef BERT_HIP_HOST_TRACE
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_call = now();
    double t_mark = t_call;
    auto lap = [&](const char *what, size_t i) { const double t = now(); fprintf(stderr, "[host] chunk %zu %-10s %.3f ms\n", i, what, t - t_mark); t_mark = t; };
#define HOST_LAP(what, i) lap(what, i)
#else
#define HOST_LAP(what, i) do { } while (0)
#endif
    HIP_OK(hipSetDevice(device_), err, -1);
    const int H = hp_.n_embd;
    // chunks [b0, b1): at most opt_.chunk_tokens tokens, at least one sentence
    struct Chunk { int b0, b1, max_len; };
    std::vector<Chunk> chunks;
    size_t max_T = 0, max_nb = 0;
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1, max_len = cu[b0 + 1] - cu[b0];
        while (b1 < B && cu[b1 + 1] - cu[b0] <= opt_.chunk_tokens) { max_len = std::max(max_len, cu[b1 + 1] - cu[b1]); ++b1; }
        chunks.push_back({b0, b1, max_len});
        max_T = std::max(max_T, (size_t)(cu[b1] - cu[b0]));
        max_nb = std::max(max_nb, (size_t)(b1 - b0));
        b0 = b1;
    }
    // every buffer is sized for the largest chunk BEFORE anything is queued: growing one later would free memory that
    // a queued chunk still uses
    const int n_slots = chunks.size() > 1 ? 2 : 1;
    auto pad16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t in_bytes = pad16(max_T * 4) + pad16((max_nb + 1) * 4) + pad16(max_nb * sizeof(int2));
    for (int i = 0; i < n_slots; ++i) {
        HostSlot &sl = slot_[i];
        const size_t in_cap = sl.h_in_cap;
        // (16 spare bytes: the staging kernel copies whole 16-byte units)
        if (!ensure_pinned((void **)&sl.h_in, &sl.h_in_cap, in_bytes + 16, err)) return -1;
        if (sl.h_in_cap != in_cap || !sl.d_in_host) HIP_OK(hipHostGetDevicePointer((void **)&sl.d_in_host, sl.h_in, 0), err, -1);
        const size_t out_cap = sl.h_out_cap;
        if (!ensure_pinned((void **)&sl.h_out, &sl.h_out_cap, max_nb * H * 4, err)) return -1;
        if (sl.h_out_cap != out_cap || !sl.d_out_host)
            HIP_OK(hipHostGetDevicePointer((void **)&sl.d_out_host, sl.h_out, 0), err, -1);
        if (!sl.d_in.ensure(in_bytes + 16, err) || (d_embeddings && !sl.d_out.ensure(max_nb * H * 4, err))) return -1;
        if (!sl.done) HIP_OK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming), err, -1);
    }
    if (!ensure_workspace((int)((max_T + 255) / 256 * 256), (int)max_nb, err)) return -1;
    HOST_LAP("prepared", (size_t)0);

    // The stream executes H2D, forward, D2H of chunk after chunk; the host runs one chunk ahead: it stages chunk i
    // into slot i & 1 and queues it, then unpacks chunk i-1 while chunk i computes.
    auto unpack = [&](size_t i) -> bool {
        HostSlot &sl = slot_[i & 1];
        if (hipEventSynchronize(sl.done) != hipSuccess) { err = "hipEventSynchronize failed"; return false; }
        HOST_LAP("wait", i);
        if (!d_embeddings) {
            const size_t bytes = (size_t)(chunks[i].b1 - chunks[i].b0) * H * 4;
            if (i + 1 == chunks.size()) copy_rows_out(embeddings + (size_t)chunks[i].b0 * H, sl.h_out, bytes);
            else memcpy(embeddings + (size_t)chunks[i].b0 * H, sl.h_out, bytes);
        }
        HOST_LAP("copy-out", i);
        return true;
    };
    auto fail = [&]() { (void)hipStreamSynchronize(stream_); return -1; };        // nothing may stay queued on the slots
    std::vector<int2> windows;
    const int slots = window_slots();                         // (once per call: the lists below and the kernels that place by them)
    const int pool_mode = pool_mode_in >= 0 ? pool_mode_in : opt_.pool_mode();      // (once per call as well: every chunk ends by the same rule)
    for (size_t i = 0; i < chunks.size(); ++i) {
        HostSlot &sl = slot_[i & 1];
        const int b0 = chunks[i].b0, nb = chunks[i].b1 - b0, T = cu[chunks[i].b1] - cu[b0];
        const size_t off_cu = pad16((size_t)T * 4), off_w = off_cu + pad16((size_t)(nb + 1) * 4);
        int32_t *h_cu = (int32_t *)(sl.h_in + off_cu);
        memcpy(sl.h_in, tokens + cu[b0], (size_t)T * 4);
        for (int j = 0; j <= nb; ++j) h_cu[j] = cu[b0 + j] - cu[b0];
        int n_windows = 0;
        if (chunks[i].max_len <= 128) {
            build_windows(h_cu, nb, windows, slots);
            n_windows = (int)windows.size();
            memcpy(sl.h_in + off_w, windows.data(), windows.size() * sizeof(int2));
        }
        const size_t staged = off_w + (size_t)n_windows * sizeof(int2);
        HOST_LAP("staged", i);
        if (opt_.stage_kernel && staged <= ((size_t)256 << 10)) {
            // (a small block — measured up to the 130 KB of a 256 x 128 batch: a few workgroups read it across the host link, the copy
            // engine's start-up is ~20 us of a 0.8 ms call; full 1 MiB chunks stay with the copy engine, off the compute stream)
            launch_stage_copy(sl.d_in_host, sl.d_in.p, staged, stream_);
        } else if (hipMemcpyAsync(sl.d_in.p, sl.h_in, staged, hipMemcpyHostToDevice, stream_) != hipSuccess) {
            err = "hipMemcpyAsync (ids) failed";
            return fail();
        }
        const char *d_in = (const char *)sl.d_in.p;
        // host destination: the pooling kernel's rows go straight into the pinned block (no D2H copy behind the pass)
        float *out = d_embeddings ? sl.d_out.as<float>() : sl.d_out_host;
        if (eval_packed_device((const int32_t *)d_in, (const int32_t *)(d_in + off_cu), nb, T, chunks[i].max_len, out, stream_, nullptr, err,
                               n_windows ? (const int2 *)(d_in + off_w) : nullptr, n_windows, slots, pool_mode) != 0)
            return fail();
        if ((d_embeddings && hipMemcpyAsync(d_embeddings + (size_t)b0 * H, sl.d_out.p, (size_t)nb * H * 4, hipMemcpyDeviceToDevice, stream_) != hipSuccess) ||
            hipEventRecord(sl.done, stream_) != hipSuccess) {
            err = "hipMemcpyAsync (embeddings) failed";
            return fail();
        }
        HOST_LAP("queued", i);
        if (i >= 1 && !unpack(i - 1)) return fail();           // while chunk i computes; frees the slot chunk i+1 stages into
    }
    if (!unpack(chunks.size() - 1)) return fail();
#undef HOST_LAP
    return 0;
}

int Engine::group_pool(const int32_t *d_cu, int B, const int32_t *d_group_cu, int n_groups, float *d_out, int pool_mode, const StreamOp &op, std::string &err) {
    const int H = hp_.n_embd;
    const hipStream_t s = op.s;
    // (2 flops per element and sentence; the launch reads B rows and writes n_groups)
    timed("group_pool", 2.0 * B * H, s, [&] {
        launch_group_pool(raw_rows_.as<float>(), (pool_mode & POOL_CLS) ? nullptr : d_cu, d_group_cu, B, n_groups, H, (pool_mode & POOL_RAW) != 0,
                          status_.as<int>(), d_out, s);
    });
    HIP_OK(hipGetLastError(), err, -1);
    return op_end(op, err) ? 0 : -1;
}

int Engine::eval_packed_grouped_device(const int32_t *d_tokens, const int32_t *d_cu, int B, int T, int max_len, const int32_t *d_group_cu,
                                       int n_groups, float *d_out, hipStream_t s, std::string &err) {
    if (B <= 0 || T <= 0 || n_groups <= 0) return 0;
    const int pool_mode = opt_.pool_mode();                   // (once per call: the pass and the pooling agree)
    HIP_OK(hipSetDevice(device_), err, -1);
    // (the pooling launch behind the pass is part of the same operation: one answer for both on whether s is capturing)
    StreamOp op;
    if (!op_begin(s, busy_, op, err)) return -1;
    if (!raw_rows_.ensure((size_t)B * hp_.n_embd * 4, err)) return -1;
    if (eval_packed_device(d_tokens, d_cu, B, T, max_len, raw_rows_.as<float>(), s, nullptr, err, nullptr, 0, 0, pool_mode | POOL_RAW) != 0) return -1;
    return group_pool(d_cu, B, d_group_cu, n_groups, d_out, pool_mode, op, err);
}

int Engine::eval_packed_grouped_host(const int32_t *tokens, const int32_t *cu, int B, const int32_t *group_cu, int n_groups, float *embeddings,
                                     float *d_embeddings, std::string &err, const float *h_raw_rows, int pool_mode_in) {
    if (B <= 0 || n_groups <= 0) return 0;
    const int pool_mode = pool_mode_in >= 0 ? pool_mode_in : opt_.pool_mode();
    const size_t H = hp_.n_embd;
    HIP_OK(hipSetDevice(device_), err, -1);
    // cu_seqlens (from 0, whatever window of the caller's prefix sums this is) | group_cu, one upload
    const size_t n_in = (size_t)B + 1 + n_groups + 1;
    if (!raw_rows_.ensure((size_t)B * H * 4, err) || !group_in_.ensure(n_in * 4, err) || (!d_embeddings && !group_out_.ensure((size_t)n_groups * H * 4, err))) return -1;
    std::vector<int32_t> in(n_in);
    for (int b = 0; b <= B; ++b) in[b] = cu[b] - cu[0];
    std::copy(group_cu, group_cu + n_groups + 1, in.begin() + B + 1);
    auto fail = [&](const char *what) { if (what) err = what; (void)hipStreamSynchronize(stream_); return -1; };      // nothing may stay queued on the caller's memory
    if (h_raw_rows) {
        // (a device-form call's pooling may still read raw_rows_ on another stream)
        if (hipStreamWaitEvent(stream_, busy_, 0) != hipSuccess || hipMemcpyAsync(raw_rows_.p, h_raw_rows, (size_t)B * H * 4, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return fail("hipMemcpyAsync (raw rows) failed");
    } else if (eval_packed_host(tokens, cu, B, nullptr, err, raw_rows_.as<float>(), pool_mode | POOL_RAW) != 0) {
        // (blocking, chunk by chunk: the rows are in raw_rows_ when it returns; they never leave the device)
        return -1;
    }
    if (hipMemcpyAsync(group_in_.p, in.data(), n_in * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) return fail("hipMemcpyAsync (groups) failed");
    float *d_out = d_embeddings ? d_embeddings : group_out_.as<float>();
    if (group_pool(group_in_.as<int32_t>(), B, group_in_.as<int32_t>() + B + 1, n_groups, d_out, pool_mode, StreamOp{stream_, busy_, false}, err) != 0) return fail(nullptr);
    if (!d_embeddings && hipMemcpyAsync(embeddings, d_out, (size_t)n_groups * H * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess)
        return fail("hipMemcpyAsync (embeddings) failed");
    HIP_OK(hipStreamSynchronize(stream_), err, -1);
    return 0;
}

int Engine::eval_packed_tokens_host(const int32_t *tokens, const int32_t *cu, int B, int flags, float *rows, float *embeddings, std::string &err) {
    if (B <= 0) return 0;
    HIP_OK(hipSetDevice(device_), err, -1);
    const size_t H = hp_.n_embd;
    auto fail = [&](const char *what) { if (what) err = what; (void)hipStreamSynchronize(stream_); return -1; };      // nothing may stay queued on the caller's memory
    // chunks [b0, b1) by eval_packed_host's rule: at most chunk_tokens tokens, at least one sentence
    std::vector<int32_t> h_cu;
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1, max_len = cu[b0 + 1] - cu[b0];
        while (b1 < B && cu[b1 + 1] - cu[b0] <= opt_.chunk_tokens) { max_len = std::max(max_len, cu[b1 + 1] - cu[b1]); ++b1; }
        const int nb = b1 - b0, T = cu[b1] - cu[b0];
        const size_t off_cu = ((size_t)T * 4 + 15) & ~(size_t)15;
        if (!tok_in_.ensure(off_cu + (size_t)(nb + 1) * 4, err) || !tok_rows_.ensure((size_t)T * H * 4, err) || !ensure_workspace((T + 255) / 256 * 256, nb, err)) return fail(nullptr);
        h_cu.resize(nb + 1);
        for (int j = 0; j <= nb; ++j) h_cu[j] = cu[b0 + j] - cu[b0];
        char *d_in = tok_in_.as<char>();
        // (pageable sources: both copies have left the host buffers when they return)
        if (hipMemcpyAsync(d_in, tokens + cu[b0], (size_t)T * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            hipMemcpyAsync(d_in + off_cu, h_cu.data(), (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return fail("hipMemcpyAsync (ids) failed");
        if (eval_packed_device((const int32_t *)d_in, (const int32_t *)(d_in + off_cu), nb, T, max_len, nullptr, stream_, nullptr, err, nullptr, 0, 0, -1,
                               tok_rows_.p, flags & TOKEN_ROWS_NORMALIZE) != 0)
            return fail(nullptr);
        if (hipMemcpyAsync(rows + (size_t)cu[b0] * H, tok_rows_.p, (size_t)T * H * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
            (embeddings && hipMemcpyAsync(embeddings + (size_t)b0 * H, d_out_.p, (size_t)nb * H * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess))
            return fail("hipMemcpyAsync (rows) failed");
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
        b0 = b1;
    }
    return 0;
}

int Engine::score_packed_device(const int32_t *d_tokens, const int32_t *d_cu, const int32_t *d_first_len, int B, int T, int max_len, int flags,
                                float *d_scores, hipStream_t s, std::string &err, const int2 *d_windows, int n_windows, int slots) {
    if (w_->n_labels <= 0) { err = "the model file has no classification head (pooler.dense.*, classifier.*)"; return -2; }
    if (B <= 0 || T <= 0) return 0;
    HIP_OK(hipSetDevice(device_), err, -1);
    // (the head launch behind the pass is part of the same operation: one answer for both on whether s is capturing)
    StreamOp op;
    if (!op_begin(s, busy_, op, err)) return -1;
    // the un-normalised [CLS] rows, in the engine's own d_out_ (ensure_workspace sizes it for the pass)
    if (eval_packed_device(d_tokens, d_cu, B, T, max_len, nullptr, s, nullptr, err, d_windows, n_windows, slots, POOL_CLS | POOL_RAW, nullptr, 0, d_first_len) != 0) return -1;
    const int H = hp_.n_embd;
    const bool f32_route = w_->f32_file && opt_.f32_exact;
    const ClsHeadArgs a{d_out_.as<float>(), w_->head_wp16.as<half_t>(), f32_route ? w_->head_wp32.as<float>() : nullptr, w_->head_bp.as<float>(),
                        w_->head_wc.as<float>(), w_->head_bc.as<float>(), d_scores, B, H, w_->n_labels, flags};
    bool ok = true;
    timed("cls_head", 2.0 * B * H * (H + w_->n_labels), s, [&] {
        ok = !f32_route && cls_head_mfma_supported(H) ? launch_cls_head(a, s) : launch_cls_head_f32(a, s);
    });
    if (!ok) { err = "cls_head: no kernel for n_embd = " + std::to_string(H); return -1; }
    HIP_OK(hipGetLastError(), err, -1);
    return op_end(op, err) ? 0 : -1;
}

int Engine::eval_packed_typed_host(const int32_t *tokens, const int32_t *cu, const int32_t *first_len, int B, bool scores, int flags, float *out,
                                   std::string &err) {
    if (scores && w_->n_labels <= 0) { err = "the model file has no classification head (pooler.dense.*, classifier.*)"; return -2; }
    if (B <= 0) return 0;
    HIP_OK(hipSetDevice(device_), err, -1);
    const size_t W = scores ? (size_t)w_->n_labels : (size_t)hp_.n_embd;      // floats per sentence that leave
    auto fail = [&](const char *what) { if (what) err = what; (void)hipStreamSynchronize(stream_); return -1; };      // nothing may stay queued on the caller's memory
    auto pad16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    // chunks [b0, b1) by eval_packed_host's rule: at most chunk_tokens tokens, at least one sentence
    std::vector<char> h_in;
    std::vector<int2> windows;
    const int slots = window_slots(), pool_mode = opt_.pool_mode();       // (once per call, as eval_packed_host reads them)
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1, max_len = cu[b0 + 1] - cu[b0];
        while (b1 < B && cu[b1 + 1] - cu[b0] <= opt_.chunk_tokens) { max_len = std::max(max_len, cu[b1 + 1] - cu[b1]); ++b1; }
        const int nb = b1 - b0, T = cu[b1] - cu[b0];
        // (the windows of eval_packed_host, so that a typed call plans as the untyped one does)
        const size_t off_cu = pad16((size_t)T * 4), off_fl = off_cu + pad16((size_t)(nb + 1) * 4), off_w = off_fl + pad16((size_t)nb * 4),
                     in_bytes = off_w + (size_t)nb * sizeof(int2);
        if (!typed_in_.ensure(in_bytes, err) || !typed_out_.ensure((size_t)nb * W * 4, err) || !ensure_workspace((T + 255) / 256 * 256, nb, err)) return fail(nullptr);
        h_in.assign(in_bytes, 0);
        memcpy(h_in.data(), tokens + cu[b0], (size_t)T * 4);
        int32_t *h_cu = (int32_t *)(h_in.data() + off_cu);
        for (int j = 0; j <= nb; ++j) h_cu[j] = cu[b0 + j] - cu[b0];
        if (first_len) memcpy(h_in.data() + off_fl, first_len + b0, (size_t)nb * 4);
        int n_windows = 0;
        if (max_len <= 128) {
            build_windows(h_cu, nb, windows, slots);
            n_windows = (int)windows.size();
            memcpy(h_in.data() + off_w, windows.data(), windows.size() * sizeof(int2));
        }
        const int2 *d_w = n_windows ? (const int2 *)(typed_in_.as<char>() + off_w) : nullptr;
        const char *d_in = typed_in_.as<char>();
        // (a pageable source: the copy has left the host buffer when it returns)
        if (hipMemcpyAsync(typed_in_.p, h_in.data(), in_bytes, hipMemcpyHostToDevice, stream_) != hipSuccess) return fail("hipMemcpyAsync (ids) failed");
        const int32_t *d_fl = first_len ? (const int32_t *)(d_in + off_fl) : nullptr;
        const int r = scores ? score_packed_device((const int32_t *)d_in, (const int32_t *)(d_in + off_cu), d_fl, nb, T, max_len, flags, typed_out_.as<float>(), stream_, err,
                                                   d_w, n_windows, slots)
                             : eval_packed_device((const int32_t *)d_in, (const int32_t *)(d_in + off_cu), nb, T, max_len, typed_out_.as<float>(), stream_, nullptr, err,
                                                  d_w, n_windows, slots, pool_mode, nullptr, 0, d_fl);
        if (r != 0) return fail(nullptr);
        if (hipMemcpyAsync(out + (size_t)b0 * W, typed_out_.p, (size_t)nb * W * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess) return fail("hipMemcpyAsync (results) failed");
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
        b0 = b1;
    }
    return 0;
}

bool Engine::ensure_sparse(int B, std::string &err) {
    sparse_chunk_ = std::max(sparse_chunk_, std::min(B, sparse_sentence_cap()));
    return sparse_dense_.ensure((size_t)sparse_chunk_ * hp_.n_vocab * 4, err);
}

int Engine::sparse_packed_device(const int32_t *d_tokens, const int32_t *d_cu, int B, int T, int max_len, int k, int32_t *d_ids, float *d_weights,
                                 hipStream_t s, std::string &err) {
    if (!w_->mlm_head) { err = "the model file has no MLM head (cls.predictions.*)"; return -2; }
    if (B <= 0 || T <= 0) return 0;
    HIP_OK(hipSetDevice(device_), err, -1);
    // (the launches behind the pass are part of the same operation: one answer for all on whether s is capturing)
    StreamOp op;
    if (!op_begin(s, busy_, op, err)) return -1;
    const int t_pad = (T + 255) / 256 * 256, H = hp_.n_embd, V = hp_.n_vocab;
    if (!ensure_workspace(t_pad, B, err) || (k > 0 && !ensure_sparse(B, err))) return -1;
    // the final states, left in x_ (its address is settled: the pass's own ensure_workspace asks for the same sizes)
    if (eval_packed_device(d_tokens, d_cu, B, T, max_len, nullptr, s, nullptr, err, nullptr, 0, 0, -1, x_.p, 0) != 0) return -1;
    const bool f32_route = w_->f32_file && opt_.f32_exact;
    const GemmWeightStore &Wt = w_->mlm_wt;
    if (f32_route) {
        timed("mlm_transform", 2.0 * T * H * H, s, [&] { launch_f32_gemm(x_.as<float>(), Wt.w.w32, w_->mlm_bt.as<float>(), nullptr, ctx_.as<float>(), T, H, H, EPI_BIAS_GELU, s); });
        timed("mlm_layernorm", 0.0, s, [&] { launch_f32_layernorm(ctx_.as<float>(), w_->mlm_ln_w.as<float>(), w_->mlm_ln_b.as<float>(), T, H, s); });
    } else {
        const bool naive = !Wt.mfma_ok || (opt_.gemm_naive && Wt.w.naive16);
        timed("mlm_transform", 2.0 * T * H * H, s, [&] {
            if (naive) launch_gemm_naive(Wt.w, x_.as<half_t>(), w_->mlm_bt.as<float>(), nullptr, ctx_.as<half_t>(), T, EPI_BIAS_GELU, s);
            else launch_gemm_mfma(Wt.w, x_.as<half_t>(), w_->mlm_bt.as<float>(), nullptr, ctx_.as<half_t>(), t_pad, EPI_BIAS_GELU, s);
        });
        timed("mlm_layernorm", 0.0, s, [&] { launch_layernorm(ctx_.as<half_t>(), w_->mlm_ln_w.as<float>(), w_->mlm_ln_b.as<float>(), T, H, s); });
    }
    const bool mfma = !f32_route && sparse_vocab_mfma_supported(H);
    SparseVocabArgs a{f32_route ? nullptr : ctx_.as<half_t>(), w_->vocab16, f32_route ? ctx_.as<float>() : nullptr, f32_route ? w_->word_emb.as<float>() : nullptr,
                      w_->mlm_bias.as<float>(), d_cu, nullptr, 0, 0, T, H, V, max_len};
    // sentences [s0, s0 + ns) -> out [ns][V]
    auto head = [&](int s0, int ns, float *out) {
        a.s0 = s0; a.ns = ns; a.out = out;
        bool ok = true;
        timed("sparse_vocab", 2.0 * T * V * H * ns / B, s, [&] { ok = mfma ? launch_sparse_vocab(a, s) : launch_sparse_vocab_f32(a, s); });
        if (ok && mfma) timed("sparse_finish", 0.0, s, [&] { launch_sparse_finish(out, (size_t)ns * V, s); });
        if (!ok) err = "sparse_vocab: no kernel for this shape (n_embd = " + std::to_string(H) + ", " + std::to_string(ns) + " sentences)";
        return ok;
    };
    if (k <= 0) {
        if (!head(0, B, d_weights)) return -1;
    } else {
        for (int s0 = 0; s0 < B; s0 += sparse_chunk_) {
            const int ns = std::min(sparse_chunk_, B - s0);
            bool ok = head(s0, ns, sparse_dense_.as<float>());
            if (ok) timed("sparse_topk", 0.0, s, [&] { ok = launch_sparse_topk(sparse_dense_.as<float>(), ns, V, k, d_ids + (size_t)s0 * k, d_weights + (size_t)s0 * k, s); });
            if (!ok) { if (err.empty()) err = "sparse_topk: no kernel for n_vocab = " + std::to_string(V) + ", k = " + std::to_string(k); return -1; }
        }
    }
    HIP_OK(hipGetLastError(), err, -1);
    return op_end(op, err) ? 0 : -1;
}

int Engine::sparse_packed_host(const int32_t *tokens, const int32_t *cu, int B, int k, int32_t *ids, float *weights, std::string &err) {
    if (!w_->mlm_head) { err = "the model file has no MLM head (cls.predictions.*)"; return -2; }
    if (B <= 0) return 0;
    HIP_OK(hipSetDevice(device_), err, -1);
    const size_t V = hp_.n_vocab, W = k > 0 ? (size_t)k : V;       // results per sentence (top-k: as many ids, then as many weights)
    const int cap = k > 0 ? std::max(1, (int)(((size_t)32 << 20) / (W * 8))) : sparse_sentence_cap();
    auto fail = [&](const char *what) { if (what) err = what; (void)hipStreamSynchronize(stream_); return -1; };      // nothing may stay queued on the caller's memory
    std::vector<int32_t> h_cu;
    for (int b0 = 0; b0 < B;) {
        int b1 = b0 + 1, max_len = cu[b0 + 1] - cu[b0];
        while (b1 < B && b1 - b0 < cap && cu[b1 + 1] - cu[b0] <= opt_.chunk_tokens) { max_len = std::max(max_len, cu[b1 + 1] - cu[b1]); ++b1; }
        const int nb = b1 - b0, T = cu[b1] - cu[b0];
        const size_t off_cu = ((size_t)T * 4 + 15) & ~(size_t)15, off_w = k > 0 ? ((size_t)nb * W * 4 + 15) & ~(size_t)15 : 0;
        if (!sparse_in_.ensure(off_cu + (size_t)(nb + 1) * 4, err) || !sparse_out_.ensure(off_w + (size_t)nb * W * 4, err)) return fail(nullptr);
        h_cu.resize(nb + 1);
        for (int j = 0; j <= nb; ++j) h_cu[j] = cu[b0 + j] - cu[b0];
        char *d_in = sparse_in_.as<char>(), *d_res = sparse_out_.as<char>();
        // (pageable sources: both copies have left the host buffers when they return)
        if (hipMemcpyAsync(d_in, tokens + cu[b0], (size_t)T * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            hipMemcpyAsync(d_in + off_cu, h_cu.data(), (size_t)(nb + 1) * 4, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return fail("hipMemcpyAsync (ids) failed");
        if (sparse_packed_device((const int32_t *)d_in, (const int32_t *)(d_in + off_cu), nb, T, max_len, k, (int32_t *)d_res, (float *)(d_res + off_w), stream_, err) != 0)
            return fail(nullptr);
        if ((k > 0 && hipMemcpyAsync(ids + (size_t)b0 * W, d_res, (size_t)nb * W * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess) ||
            hipMemcpyAsync(weights + (size_t)b0 * W, d_res + off_w, (size_t)nb * W * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess)
            return fail("hipMemcpyAsync (results) failed");
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
        b0 = b1;
    }
    return 0;
}

int Engine::eval_hidden(const int32_t *tokens, int N, float *hidden, float *embedding, std::string &err) {
    HIP_OK(hipSetDevice(device_), err, -1);
    const int H = hp_.n_embd, L = hp_.n_layer;
    int32_t cu[2] = {0, N};
    if (!d_tokens_.ensure((size_t)N * 4, err) || !d_cu_.ensure(8, err)) return -1;
    if (!d_hidden_.ensure((size_t)(L + 1) * N * H * 4, err)) return -1;
    const int t_pad = (N + 255) / 256 * 256;
    if (!ensure_workspace(t_pad, 1, err)) return -1;
    HIP_OK(hipMemcpy(d_tokens_.p, tokens, (size_t)N * 4, hipMemcpyHostToDevice), err, -1);
    HIP_OK(hipMemcpy(d_cu_.p, cu, 8, hipMemcpyHostToDevice), err, -1);
    if (eval_packed_device(d_tokens_.as<int32_t>(), d_cu_.as<int32_t>(), 1, N, N, d_out_.as<float>(), stream_,
                           d_hidden_.as<float>(), err) != 0)
        return -1;
    HIP_OK(hipStreamSynchronize(stream_), err, -1);
    if (hidden) HIP_OK(hipMemcpy(hidden, d_hidden_.p, (size_t)(L + 1) * N * H * 4, hipMemcpyDeviceToHost), err, -1);
    if (embedding) HIP_OK(hipMemcpy(embedding, d_out_.p, (size_t)H * 4, hipMemcpyDeviceToHost), err, -1);
    return 0;
}

}  // namespace bert_hip
