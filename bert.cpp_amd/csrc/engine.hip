// engine.hip — see engine.h: creation, the workspace, plan(), the routes and the device forms (the host forms: engine_host.cpp).
#include "engine.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
    lo.naive = e->opt_.gemm_naive; lo.expand_q4 = e->opt_.q4_expand; lo.ln_fold = e->opt_.ln_fold; lo.mx = e->opt_.mx_load;
    e->w_ = ModelWeights::load(mf, lo, err);
    if (!e->w_ || !e->status_.alloc(16, err)) return nullptr;
    e->opt_.mx = e->w_->mx_images();                          // (the route is the default of a load that built its images)
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
    if (!test_poison_option(key, ctx_, y_, {&x_, &qkv_, &ctx_, &y_, &ff_, &v32_, &ln_stats1_, &ln_stats2_, &ln_rows1_, &ln_rows2_, &d_hidden_, &mx_a_, &mx_b_})) opt_.set(key, value, w_->naive_images(), w_->fold_images, w_->mx_images());
}

bool Engine::ensure_workspace(int t_pad, int n_sentences, std::string &err) {
    const size_t H = hp_.n_embd, I = hp_.n_intermediate, tp = (size_t)t_pad;
    const size_t es = w_->f32_file ? 4 : 2;                      // (f32 files: the f32 route's activations are f32)
    return x_.ensure(tp * H * es, err) && qkv_.ensure(tp * 3 * H * es, err) && ctx_.ensure(tp * H * es, err) &&
           y_.ensure(tp * H * es, err) && ff_.ensure(tp * I * es, err) && v32_.ensure((size_t)std::max(128, std::min(t_pad, (opt_.latency_tokens + 255) / 256 * 256)) * H * 4, err) &&
           d_out_.ensure((size_t)n_sentences * H * 4, err) &&
           windows_.ensure((size_t)n_sentences * sizeof(int2), err) &&
           (!w_->mx_images() || (mx_a_.ensure(MxRows::bytes(t_pad, (int)std::max(H, I)), err) && mx_b_.ensure(MxRows::bytes(t_pad, (int)std::max(H, I)), err))) &&
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

int Engine::eval_packed_device(const Pass &pass, std::string &err) {
    const int B = pass.n_sentences, T = pass.n_tokens, max_len = pass.max_len;
    const int32_t *d_tokens = pass.d_tokens, *d_cu = pass.d_cu, *d_first_len = pass.d_first_len;
    const hipStream_t s = pass.stream;
    if (B <= 0 || T <= 0) return 0;
    // the windows' place granularity, read ONCE per pass (the host path read it when it built its list): the window list, the
    // grid bound and the kernels' place rule must agree whatever another thread or context sets meanwhile
    const int slots = pass.window_slots ? pass.window_slots : window_slots();
    // (so are "pooling" and "normalize": every launch that ends the pass gets the plan's value)
    const int pool_mode = pass.pool_mode >= 0 ? pass.pool_mode : opt_.pool_mode();
    HIP_OK(hipSetDevice(device_), err, -1);
    // one forward pass at a time on the shared workspace: wait (on the caller's stream) for the previous pass — unless s is capturing
    StreamOp op;
    if (!op_begin(s, busy_, op, err)) return -1;
    if (!ensure_workspace((T + 255) / 256 * 256, B, err)) return -1;
    prof_.begin_pass();
    // (a token-rows call that wants no embeddings: ensure_workspace sized d_out_)
    float *d_out = pass.d_out ? pass.d_out : d_out_.as<float>();
    const Plan p = plan(pass, slots, pool_mode, d_out);
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
    // (the projection head in token_rows' place: the same states, [T][token_dim] rows; the callers refused the f32 route and a file without a head)
    if (pass.d_token_rows && (pass.token_flags & TOKEN_ROWS_PROJECT)) {
        if (p.route == Route::F32 || w_->token_dim <= 0 || !token_project_supported(hp_.n_embd, w_->token_dim)) { err = "token_project: no projection head, or the f32 route"; return -1; }
        timed("token_project", 2.0 * T * hp_.n_embd * w_->token_dim, s, [&] { launch_token_project(x_.as<half_t>(), w_->token_proj.as<half_t>(), T, hp_.n_embd, w_->token_dim, d_cu, B, max_len, pass.token_flags, pass.d_token_rows, s); });
    } else if (pass.d_token_rows && pass.d_token_rows != x_.p)
        timed("token_rows", 0.0, s, [&] { launch_token_rows(x_.p, p.route == Route::F32, T, hp_.n_embd, d_cu, B, max_len, pass.token_flags, pass.d_token_rows, s); });
    HIP_OK(hipGetLastError(), err, -1);
    return op_end(op, err) ? 0 : -1;
}

// The route of a pass and, per layer, its kernels: every eligibility test of the forward pass, each made here once.  Launches nothing.
Engine::Plan Engine::plan(const Pass &pass, int slots, int pool_mode, float *d_out) const {
    const int B = pass.n_sentences, T = pass.n_tokens, max_len = pass.max_len, n_windows = pass.n_windows;
    const int2 *d_windows = pass.d_windows;
    // (t_pad: whole tiles of every kernel family, 128- and 256-token tiles)
    Plan p{pass, (T + 255) / 256 * 256, slots, pool_mode, d_out, d_windows, n_windows};
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
    // The MXFP8 route, where the load built the images and "mx" is on: every layer as mat-muls of gemm_mx.hip around the attention and
    // LayerNorm launches — x materialised after every layer, so taps and token rows are served —, ahead of every other f16 route
    bool mx = opt_.mx && mx_a_.p && mx_b_.p;
    for (int il = 0; mx && il < Lz; ++il) {
        const LayerWeights &L = w_->layers[il];
        mx = gemm_mx_supported(L.qkv.w, p.t_pad) && gemm_mx_supported(L.o.w, p.t_pad) && gemm_mx_supported(L.ffi.w, p.t_pad) && gemm_mx_supported(L.ffo.w, p.t_pad);
    }
    if (mx) {
        for (LayerPlan &lp : p.layers) { lp = LayerPlan(); lp.qkv = lp.o = lp.ffi = lp.ffo = Family::MX; }
        p.route = Route::LAYERED;
        return p;
    }
    // a hidden-state tap wants every layer's normalised states: it takes neither the one-launch kernel nor the folded LayerNorms
    if (pass.d_hidden) one_launch = fold = false;
    // token rows want the last layer's states in x_ in row order: not the one-launch kernel; the folded LayerNorms stay
    if (pass.d_token_rows) one_launch = false;
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
        timed(name, 2.0 * p.pass.n_tokens * W.w.N * W.w.K, p.pass.stream, [&] {
            if (f == Family::F32) launch_f32_gemm((const float *)A, W.w.w32, bias, (const float *)resid, (float *)C, p.pass.n_tokens, W.w.N, W.w.K, epi, p.pass.stream);
            else if (f == Family::GEMM256) ok = launch_gemm256(W.w, a, bias, r, (half_t *)C, p.t_pad, epi, p.pass.stream, ln);
            else if (f == Family::MFMA) launch_gemm_mfma(W.w, a, bias, r, (half_t *)C, p.t_pad, epi, p.pass.stream);
            else launch_gemm_naive(W.w, a, bias, r, (half_t *)C, p.pass.n_tokens, epi, p.pass.stream);
        });
    if (!ok) err = std::string(name) + ": no " + kernel[(int)f] + " kernel for LayerNorm-folding flags " + std::to_string(ln->flags) + ", epilogue " + std::to_string(epi);
    return ok;
}

void Engine::mx_quantize(const Plan &p, const half_t *x, int K, const MxRows &out) {
    timed("mx_quantize", 0.0, p.pass.stream, [&] { launch_mx_quantize_rows(x, p.pass.n_tokens, p.t_pad, K, out, p.pass.stream); });
}

void Engine::gemm_mx(const Plan &p, const char *name, const GemmWeightStore &W, const MxRows &A, const float *bias, const half_t *resid, half_t *C16,
                     MxRows *Cmx, int epi) {
    prof_.count_family("family:gemm_mx");
    timed(name, 2.0 * p.pass.n_tokens * W.w.N * W.w.K, p.pass.stream, [&] { launch_gemm_mx(W.w, A, bias, resid, C16, Cmx, p.t_pad, epi, p.pass.stream); });
}

// A layer of the MXFP8 route: every mat-mul reads MX rows.  The inputs other kernels produce (x, the attention context, LayerNorm's y)
// pass the row quantiser; the up-projection writes its GELU output as MX rows itself, so the intermediate never exists in f16.
void Engine::forward_layer_mx(const Plan &p, const LayerWeights &L) {
    const int H = hp_.n_embd, I = hp_.n_intermediate;
    half_t *x = x_.as<half_t>(), *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>(), *y = y_.as<half_t>();
    const MxRows a{mx_a_.as<uint8_t>(), p.t_pad, H};
    MxRows ff{mx_b_.as<uint8_t>(), p.t_pad, I};
    mx_quantize(p, x, H, a);
    gemm_mx(p, "gemm_qkv", L.qkv, a, L.qkv_b.as<float>(), nullptr, qkv, nullptr, EPI_BIAS);
    attention(p);
    mx_quantize(p, ctx, H, a);
    gemm_mx(p, "gemm_attn_out", L.o, a, L.o_b.as<float>(), x, y, nullptr, EPI_BIAS_RESID);
    timed("layernorm", 0.0, p.pass.stream, [&] { launch_layernorm(y, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
    mx_quantize(p, y, H, a);
    gemm_mx(p, "gemm_ffn_up", L.ffi, a, L.ffi_b.as<float>(), nullptr, nullptr, &ff, EPI_BIAS_GELU);
    gemm_mx(p, "gemm_ffn_down", L.ffo, ff, L.ffo_b.as<float>(), y, x, nullptr, EPI_BIAS_RESID);
    timed("layernorm", 0.0, p.pass.stream, [&] { launch_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
}

// (attention FLOPs: 4 * sum_b N_b^2 * H; only T and max_len are known here -> upper bound T * max_len)
void Engine::attention(const Plan &p) {
    const int H = hp_.n_embd, nh = hp_.n_head, dh = H / nh;
    half_t *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>();
    // (the relative position bias of the file, if it has one: null pointers otherwise)
    const int P = hp_.n_max_tokens;
    timed("attention", 4.0 * p.pass.n_tokens * p.pass.max_len * H, p.pass.stream, [&] {
        if (opt_.attn_naive || !launch_attention_mfma(qkv, p.pass.d_cu, p.pass.n_sentences, nh, dh, p.pass.max_len, ctx, p.pass.stream, w_->rel_scaled.as<float>(), P))
            launch_attention_naive(qkv, p.pass.d_cu, p.pass.n_sentences, nh, dh, p.pass.max_len, ctx, p.pass.stream, w_->rel.as<float>(), P);
    });
}

// the layer states of eval_hidden as f32: x after the embedding LayerNorm (idx 0) and after every layer
void Engine::tap(const Plan &p, int idx) {
    const size_t n = (size_t)p.pass.n_tokens * hp_.n_embd;
    if (p.pass.d_hidden && p.route == Route::F32) (void)hipMemcpyAsync(p.pass.d_hidden + idx * n, x_.p, n * 4, hipMemcpyDeviceToDevice, p.pass.stream);
    else if (p.pass.d_hidden) launch_f16_to_f32(x_.as<half_t>(), p.pass.d_hidden + idx * n, n, p.pass.stream);
}

// The latency route (skinny.hip): a call of a few windows would keep as many CUs of 256 busy on the fused kernels.  Same bits per
// sentence (the route must not show in the results), seven short launches per layer.
void Engine::forward_latency(const Plan &p) {
    const int H = hp_.n_embd, I = hp_.n_intermediate, tb = (p.pass.n_tokens + 31) / 32, Lz = hp_.n_layer;
    half_t *x = x_.as<half_t>(), *qkv = qkv_.as<half_t>(), *ctx = ctx_.as<half_t>(), *y = y_.as<half_t>(), *ff = ff_.as<half_t>();
    float *v32 = v32_.as<float>();
    for (int il = 0; il < Lz; ++il) {
        const LayerWeights &L = w_->layers[il];
        // (from the second layer on the QKV kernel LayerNorms the previous layer's output itself and writes x)
        const LayerWeights *P = il ? &w_->layers[il - 1] : nullptr;
        timed("skinny_qkv", 2.0 * p.pass.n_tokens * 3 * H * H, p.pass.stream, [&] {
            launch_skinny_gemm(0, L.qkv.w, x, P ? v32 : nullptr, P ? P->ln_out_w.as<float>() : nullptr, P ? P->ln_out_b.as<float>() : nullptr,
                               x, L.qkv_b.as<float>(), nullptr, qkv, nullptr, tb, p.pass.stream);
        });
        attention(p);
        timed("skinny_proj", 2.0 * p.pass.n_tokens * H * H, p.pass.stream, [&] {
            launch_skinny_gemm(1, L.o.w, ctx, nullptr, nullptr, nullptr, nullptr, L.o_b.as<float>(), x, nullptr, v32, tb, p.pass.stream);
        });
        timed("skinny_ffn_up", 2.0 * p.pass.n_tokens * H * I, p.pass.stream, [&] {
            launch_skinny_gemm(2, L.ffi.w, nullptr, v32, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), y, L.ffi_b.as<float>(), nullptr, ff, nullptr, tb, p.pass.stream);
        });
        timed("skinny_ffn_down", 2.0 * p.pass.n_tokens * H * I, p.pass.stream, [&] {
            launch_skinny_gemm(3, L.ffo.w, ff, nullptr, nullptr, nullptr, nullptr, L.ffo_b.as<float>(), y, nullptr, v32, tb, p.pass.stream);
        });
        // (the last layer, or a hidden-state tap: somebody has to materialise x now; the next QKV kernel writes the same bits again)
        if (il + 1 == Lz || p.pass.d_hidden)
            timed("skinny_layernorm", 0.0, p.pass.stream, [&] { launch_skinny_layernorm(v32, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), x, tb, H, p.pass.stream); });
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
    timed("model_kernel", hp_.n_layer * (2.0 * p.pass.n_tokens * 3 * H * H + 4.0 * p.pass.n_tokens * p.pass.max_len * H + 2.0 * p.pass.n_tokens * H * H + 4.0 * p.pass.n_tokens * H * I), p.pass.stream, [&] {
        launch_model_kernel(mw, hp_.n_layer, x_.as<half_t>(), ctx_.as<half_t>(), y_.as<half_t>(), p.pass.d_cu, p.pass.n_sentences, p.pass.n_tokens, p.windows, p.n_windows, p.n_windows_dev, hp_.n_head,
                            p.out, p.pass.max_len, status_.as<int>(), p.pool_mode, p.slots, p.pass.stream);
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
        timed("ln_rows_finalize", 0.0, p.pass.stream, [&] { launch_ln_rows_finalize(st1, P, p.t_pad, H, rows1, p.pass.stream); });
        ln = GemmLnFold(); ln.flags = GemmLnFold::IN; ln.rows_in = rows1; ln.waug = L.ffi_waug.as<half_t>();
        if (!gemm(p, "gemm_ffn_up", G, L.ffi_fold, y, nullptr, nullptr, ff, EPI_BIAS_GELU, err, &ln)) return false;
        // u2 = ff W2^T + b2 + LayerNorm(u1) -> x
        ln = GemmLnFold(); ln.flags = GemmLnFold::STATS | GemmLnFold::RES; ln.stats = st2; ln.rows_res = rows1; ln.gb = L.ffo_gb.as<unsigned>();
        if (!gemm(p, "gemm_ffn_down", G, L.ffo, ff, L.ffo_b.as<float>(), y, x, EPI_BIAS_RESID, err, &ln)) return false;
        timed("ln_rows_finalize", 0.0, p.pass.stream, [&] { launch_ln_rows_finalize(st2, P, p.t_pad, H, rows2, p.pass.stream); });
        if (il + 1 == hp_.n_layer)     // (the pooling reads normalised rows: the one LayerNorm launch of the pass)
            timed("layernorm", 0.0, p.pass.stream, [&] { launch_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
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
        if (lp.qkv == Family::MX) {
            forward_layer_mx(p, L);
            tap(p, il + 1);
            continue;
        }
        if (lp.qkv2) {
            // windows of 128 token slots holding whole sentences: Q|K|V never reach HBM whatever the sentence lengths
            timed("qkv_attention2", 2.0 * p.pass.n_tokens * L.qkv.w.N * L.qkv.w.K + 4.0 * p.pass.n_tokens * p.pass.max_len * H, p.pass.stream, [&] {
                launch_qkv_attention2(L.qkv.w, x, L.qkv_b.as<float>(), p.pass.d_cu, p.pass.n_sentences, p.windows, p.n_windows, p.n_windows_dev, p.pass.max_len, hp_.n_head, p.slots, ctx, p.pass.stream);
            });
        } else {
            if (!gemm(p, "gemm_qkv", lp.qkv, lp.planes ? L.qkv_q4 : L.qkv, x, L.qkv_b.as<float>(), nullptr, qkv, EPI_BIAS, err)) return false;
            attention(p);
        }
        if (lp.tail) {
            // out-projection + LN + FFN + LN in one launch, a pair of specialist waves per 32 tokens: y and the intermediate never leave the chip
            timed("layer_tail", 2.0 * p.pass.n_tokens * H * H + 4.0 * p.pass.n_tokens * H * I, p.pass.stream, [&] {
                launch_layer_tail(L.o.w, L.ffi.w, L.ffo.w, ctx, x, L.o_b.as<float>(), L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), L.ffi_b.as<float>(),
                                  L.ffo_b.as<float>(), L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), x, p.t_pad, p.pass.stream);
            });
        } else {
            if (!gemm(p, "gemm_attn_out", lp.o, L.o, ctx, L.o_b.as<float>(), x, y, EPI_BIAS_RESID, err)) return false;
            timed("layernorm", 0.0, p.pass.stream, [&] { launch_layernorm(y, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
            if (!gemm(p, "gemm_ffn_up", lp.ffi, L.ffi, y, L.ffi_b.as<float>(), nullptr, ff, EPI_BIAS_GELU, err) ||
                !gemm(p, "gemm_ffn_down", lp.ffo, L.ffo, ff, L.ffo_b.as<float>(), y, x, EPI_BIAS_RESID, err)) return false;
            timed("layernorm", 0.0, p.pass.stream, [&] { launch_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
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
    timed("embed_ln", 0.0, p.pass.stream, [&] {
        launch_f32_embed_ln(w_->word_emb.as<float>(), w_->type_emb.as<float>(), w_->pos_emb.as<float>(), w_->ln_e_w.as<float>(), w_->ln_e_b.as<float>(), p.pass.d_tokens,
                            p.pass.d_cu, p.pass.n_sentences, p.pass.n_tokens, H, hp_.n_vocab, p.pass.max_len, x, p.pass.stream, p.pass.d_first_len);
    });
    tap(p, 0);
    for (int il = 0; il < hp_.n_layer; ++il) {
        const LayerWeights &L = w_->layers[il];
        if (!gemm(p, "gemm_qkv", F, L.qkv, x, L.qkv_b.as<float>(), nullptr, qkv, EPI_BIAS, err)) return false;
        bool launched = true;
        timed("attention", 4.0 * p.pass.n_tokens * p.pass.max_len * H, p.pass.stream, [&] { launched = launch_f32_attention(qkv, p.pass.d_cu, p.pass.n_sentences, nh, dh, p.pass.max_len, ctx, p.pass.stream, w_->rel.as<float>(), hp_.n_max_tokens); });
        if (!launched) {
            err = "f32 route: the attention kernel keeps the scores of max_len = " + std::to_string(p.pass.max_len) + " keys per wave in LDS, " +
                  std::to_string(f32_attention_lds_bytes(p.pass.max_len)) + " bytes a workgroup; this device's limit is " +
                  std::to_string(f32_attention_lds_limit()) + " bytes (set_option \"f32\" = \"f16\" selects the f16 kernels)";
            return false;
        }
        if (!gemm(p, "gemm_attn_out", F, L.o, ctx, L.o_b.as<float>(), x, y, EPI_BIAS_RESID, err)) return false;
        timed("layernorm", 0.0, p.pass.stream, [&] { launch_f32_layernorm(y, L.ln_att_w.as<float>(), L.ln_att_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
        if (!gemm(p, "gemm_ffn_up", F, L.ffi, y, L.ffi_b.as<float>(), nullptr, ff, EPI_BIAS_GELU, err) ||
            !gemm(p, "gemm_ffn_down", F, L.ffo, ff, L.ffo_b.as<float>(), y, x, EPI_BIAS_RESID, err)) return false;
        timed("layernorm", 0.0, p.pass.stream, [&] { launch_f32_layernorm(x, L.ln_out_w.as<float>(), L.ln_out_b.as<float>(), p.pass.n_tokens, H, p.pass.stream); });
        tap(p, il + 1);
    }
    timed("pool_normalize", 2.0 * p.pass.n_tokens * H, p.pass.stream, [&] { launch_f32_pool_normalize(x, p.pass.d_cu, p.pass.n_sentences, H, p.pass.max_len, status_.as<int>(), p.out, p.pool_mode, p.pass.stream); });
    return true;
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
    Pass pass;
    pass.d_tokens = d_tokens; pass.d_cu = d_cu; pass.n_sentences = B; pass.n_tokens = T; pass.max_len = max_len; pass.stream = s;
    pass.d_out = raw_rows_.as<float>();
    pass.pool_mode = pool_mode | POOL_RAW;
    if (eval_packed_device(pass, err) != 0) return -1;
    return group_pool(d_cu, B, d_group_cu, n_groups, d_out, pool_mode, op, err);
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
    Pass pass;
    pass.d_tokens = d_tokens; pass.d_cu = d_cu; pass.n_sentences = B; pass.n_tokens = T; pass.max_len = max_len; pass.stream = s;
    pass.d_windows = d_windows; pass.n_windows = n_windows; pass.window_slots = slots;
    pass.pool_mode = POOL_CLS | POOL_RAW;
    pass.d_first_len = d_first_len;
    if (eval_packed_device(pass, err) != 0) return -1;
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
    Pass pass;
    pass.d_tokens = d_tokens; pass.d_cu = d_cu; pass.n_sentences = B; pass.n_tokens = T; pass.max_len = max_len; pass.stream = s;
    pass.d_token_rows = x_.p;
    if (eval_packed_device(pass, err) != 0) return -1;
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

}  // namespace bert_hip
