// engine_host.cpp — the host side of the engine (engine.h): the entry points that take a batch in host memory.  They cut it by the
// chunk rule and stage a chunk by the layout of host_chunks.h: eval_packed_host pipelined through two pinned slots, the typed,
// token-rows and sparse forms blocking on every chunk (blocking_host_chunks).
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <system_error>
#include <thread>

#include "host_chunks.h"

namespace bert_hip {

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
    // the chunks (host_chunks.h: the chunk rule), all of them up front
    std::vector<HostChunk> chunks;
    size_t max_T = 0, max_nb = 0;
    for (int b0 = 0; b0 < B; b0 = chunks.back().b1) {
        chunks.push_back(next_host_chunk(cu, B, b0, opt_.chunk_tokens, 0));
        max_T = std::max(max_T, (size_t)(cu[chunks.back().b1] - cu[b0]));
        max_nb = std::max(max_nb, (size_t)(chunks.back().b1 - b0));
    }
    // every buffer is sized for the largest chunk BEFORE anything is queued: growing one later would free memory that
    // a queued chunk still uses
    const int n_slots = chunks.size() > 1 ? 2 : 1;
    const size_t in_bytes = StagingLayout(max_T, max_nb, false, max_nb).bytes;
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
        const HostChunk &c = chunks[i];
        const int b0 = c.b0, nb = c.b1 - b0, T = cu[c.b1] - cu[b0];
        windows.clear();
        if (c.max_len <= 128) build_windows(cu + b0, nb, windows, slots);
        const int n_windows = (int)windows.size();
        const StagingLayout L(T, nb, false, n_windows);
        fill_staging(sl.h_in, L, tokens, cu, c, nullptr, windows.data(), n_windows);
        HOST_LAP("staged", i);
        if (opt_.stage_kernel && L.bytes <= ((size_t)256 << 10)) {
            // (a small block — measured up to the 130 KB of a 256 x 128 batch: a few workgroups read it across the host link, the copy
            // engine's start-up is ~20 us of a 0.8 ms call; full 1 MiB chunks stay with the copy engine, off the compute stream)
            launch_stage_copy(sl.d_in_host, sl.d_in.p, L.bytes, stream_);
        } else if (hipMemcpyAsync(sl.d_in.p, sl.h_in, L.bytes, hipMemcpyHostToDevice, stream_) != hipSuccess) {
            err = "hipMemcpyAsync (ids) failed";
            return fail();
        }
        const char *d_in = (const char *)sl.d_in.p;
        Pass pass;
        pass.d_tokens = (const int32_t *)d_in; pass.d_cu = (const int32_t *)(d_in + L.off_cu);
        pass.n_sentences = nb; pass.n_tokens = T; pass.max_len = c.max_len; pass.stream = stream_;
        // host destination: the pooling kernel's rows go straight into the pinned block (no D2H copy behind the pass)
        pass.d_out = d_embeddings ? sl.d_out.as<float>() : sl.d_out_host;
        pass.d_windows = n_windows ? (const int2 *)(d_in + L.off_windows) : nullptr; pass.n_windows = n_windows; pass.window_slots = slots;
        pass.pool_mode = pool_mode;
        if (eval_packed_device(pass, err) != 0) return fail();
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

// The walk of the three blocking chunked forms.  Per chunk (the chunk rule under max_sentences): out_bytes(nb, T) bytes of host_out_, the
// staging block filled in host_block_ and sent to host_in_ by one copy (a pageable source: the copy has left the block when it returns),
// then queue(chunk, pass) — pass: the chunk's ids, cu_seqlens, sizes, first_len and windows on stream_ — queues the pass and the copies
// back (false + err).  slots > 0: with the windows of eval_packed_host, so that the call plans as eval_packed_host's does.  The stream
// is drained behind every chunk and on every failure: nothing stays queued on the caller's memory or on the one pair of buffers.
template <class OutBytes, class Queue>
int Engine::blocking_host_chunks(const int32_t *tokens, const int32_t *cu, const int32_t *first_len, int B, int max_sentences, int slots, OutBytes &&out_bytes,
                                 Queue &&queue, std::string &err) {
    HIP_OK(hipSetDevice(device_), err, -1);
    auto fail = [&](const char *what) { if (what) err = what; (void)hipStreamSynchronize(stream_); return -1; };
    std::vector<int2> windows;
    for (int b0 = 0; b0 < B;) {
        const HostChunk c = next_host_chunk(cu, B, b0, opt_.chunk_tokens, max_sentences);
        const int nb = c.b1 - b0, T = cu[c.b1] - cu[b0];
        windows.clear();
        if (slots > 0 && c.max_len <= 128) build_windows(cu + b0, nb, windows, slots);
        const StagingLayout L(T, nb, first_len != nullptr, windows.size());
        if (!host_in_.ensure(L.bytes, err) || !host_out_.ensure(out_bytes(nb, T), err) || !ensure_workspace((T + 255) / 256 * 256, nb, err)) return fail(nullptr);
        host_block_.resize(std::max(host_block_.size(), L.bytes));
        fill_staging(host_block_.data(), L, tokens, cu, c, first_len, windows.data(), windows.size());
        if (hipMemcpyAsync(host_in_.p, host_block_.data(), L.bytes, hipMemcpyHostToDevice, stream_) != hipSuccess) return fail("hipMemcpyAsync (ids) failed");
        const char *d_in = host_in_.as<char>();
        Pass pass;
        pass.d_tokens = (const int32_t *)d_in; pass.d_cu = (const int32_t *)(d_in + L.off_cu);
        pass.n_sentences = nb; pass.n_tokens = T; pass.max_len = c.max_len; pass.stream = stream_;
        pass.d_first_len = first_len ? (const int32_t *)(d_in + L.off_first_len) : nullptr;
        pass.d_windows = windows.empty() ? nullptr : (const int2 *)(d_in + L.off_windows); pass.n_windows = (int)windows.size(); pass.window_slots = slots;
        if (!queue(c, pass)) return fail(nullptr);
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
        b0 = c.b1;
    }
    return 0;
}

int Engine::eval_packed_grouped_host(const int32_t *tokens, const int32_t *cu, int B, const int32_t *group_cu, int n_groups, float *embeddings,
                                     float *d_embeddings, std::string &err, const float *h_raw_rows, int pool_mode_in) {
    if (B <= 0 || n_groups <= 0) return 0;
    const int pool_mode = pool_mode_in >= 0 ? pool_mode_in : opt_.pool_mode();
    const size_t H = hp_.n_embd;
    HIP_OK(hipSetDevice(device_), err, -1);
    // cu_seqlens (from 0, whatever window of the caller's prefix sums this is) | group_cu, one upload
    const size_t n_in = (size_t)B + 1 + n_groups + 1;
    if (!raw_rows_.ensure((size_t)B * H * 4, err) || !host_in_.ensure(n_in * 4, err) || (!d_embeddings && !host_out_.ensure((size_t)n_groups * H * 4, err))) return -1;
    std::vector<int32_t> in(n_in);
    for (int b = 0; b <= B; ++b) in[b] = cu[b] - cu[0];
    std::copy(group_cu, group_cu + n_groups + 1, in.begin() + B + 1);
    auto fail = [&](const char *what) { if (what) err = what; (void)hipStreamSynchronize(stream_); return -1; };      // nothing may stay queued on the caller's memory
    if (h_raw_rows) {
        // (a device-form call's pooling may still read raw_rows_ on another stream)
        if (hipStreamWaitEvent(stream_, busy_, 0) != hipSuccess || hipMemcpyAsync(raw_rows_.p, h_raw_rows, (size_t)B * H * 4, hipMemcpyHostToDevice, stream_) != hipSuccess)
            return fail("hipMemcpyAsync (raw rows) failed");
    } else if (eval_packed_host(tokens, cu, B, nullptr, err, raw_rows_.as<float>(), pool_mode | POOL_RAW) != 0) {
        // (blocking, chunk by chunk through the pinned slots: the rows are in raw_rows_ when it returns; they never leave the device)
        return -1;
    }
    if (hipMemcpyAsync(host_in_.p, in.data(), n_in * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) return fail("hipMemcpyAsync (groups) failed");
    float *d_out = d_embeddings ? d_embeddings : host_out_.as<float>();
    if (group_pool(host_in_.as<int32_t>(), B, host_in_.as<int32_t>() + B + 1, n_groups, d_out, pool_mode, StreamOp{stream_, busy_, false}, err) != 0) return fail(nullptr);
    if (!d_embeddings && hipMemcpyAsync(embeddings, d_out, (size_t)n_groups * H * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess)
        return fail("hipMemcpyAsync (embeddings) failed");
    HIP_OK(hipStreamSynchronize(stream_), err, -1);
    return 0;
}

int Engine::eval_packed_tokens_host(const int32_t *tokens, const int32_t *cu, int B, int flags, float *rows, float *embeddings, std::string &err) {
    if (B <= 0) return 0;
    // (W: values per row — the projection head's under TOKEN_ROWS_PROJECT; H: per embedding)
    const size_t H = hp_.n_embd, W = flags & TOKEN_ROWS_PROJECT ? (size_t)w_->token_dim : H;
    return blocking_host_chunks(tokens, cu, nullptr, B, 0, 0, [&](int, int T) { return (size_t)T * W * 4; }, [&](const HostChunk &c, Pass &pass) {
        pass.d_token_rows = host_out_.p; pass.token_flags = flags & (TOKEN_ROWS_NORMALIZE | TOKEN_ROWS_PROJECT);
        if (eval_packed_device(pass, err) != 0) return false;
        if (hipMemcpyAsync(rows + (size_t)cu[c.b0] * W, host_out_.p, (size_t)pass.n_tokens * W * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess &&
            (!embeddings || hipMemcpyAsync(embeddings + (size_t)c.b0 * H, d_out_.p, (size_t)pass.n_sentences * H * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess))
            return true;
        err = "hipMemcpyAsync (rows) failed";
        return false;
    }, err);
}

int Engine::eval_packed_typed_host(const int32_t *tokens, const int32_t *cu, const int32_t *first_len, int B, bool scores, int flags, float *out,
                                   std::string &err) {
    if (scores && w_->n_labels <= 0) { err = "the model file has no classification head (pooler.dense.*, classifier.*)"; return -2; }
    if (B <= 0) return 0;
    const size_t W = scores ? (size_t)w_->n_labels : (size_t)hp_.n_embd;      // floats per sentence that leave
    const int slots = window_slots(), pool_mode = opt_.pool_mode();       // (once per call, as eval_packed_host reads them)
    return blocking_host_chunks(tokens, cu, first_len, B, 0, slots, [&](int nb, int) { return (size_t)nb * W * 4; }, [&](const HostChunk &c, Pass &pass) {
        const int nb = pass.n_sentences;
        pass.d_out = host_out_.as<float>(); pass.pool_mode = pool_mode;
        const int r = scores ? score_packed_device(pass.d_tokens, pass.d_cu, pass.d_first_len, nb, pass.n_tokens, c.max_len, flags, host_out_.as<float>(), stream_, err,
                                                   pass.d_windows, pass.n_windows, slots)
                             : eval_packed_device(pass, err);
        if (r != 0) return false;
        if (hipMemcpyAsync(out + (size_t)c.b0 * W, host_out_.p, (size_t)nb * W * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess) return true;
        err = "hipMemcpyAsync (results) failed";
        return false;
    }, err);
}

int Engine::sparse_packed_host(const int32_t *tokens, const int32_t *cu, int B, int k, int32_t *ids, float *weights, std::string &err) {
    if (!w_->mlm_head) { err = "the model file has no MLM head (cls.predictions.*)"; return -2; }
    if (B <= 0) return 0;
    const size_t V = hp_.n_vocab, W = k > 0 ? (size_t)k : V;       // results per sentence (top-k: as many ids, then as many weights)
    const int cap = k > 0 ? std::max(1, (int)(((size_t)32 << 20) / (W * 8))) : sparse_sentence_cap();
    auto off_w = [&](int nb) { return k > 0 ? ((size_t)nb * W * 4 + 15) & ~(size_t)15 : (size_t)0; };
    return blocking_host_chunks(tokens, cu, nullptr, B, cap, 0, [&](int nb, int) { return off_w(nb) + (size_t)nb * W * 4; }, [&](const HostChunk &c, Pass &pass) {
        const int nb = pass.n_sentences;
        char *d_res = host_out_.as<char>();
        if (sparse_packed_device(pass.d_tokens, pass.d_cu, nb, pass.n_tokens, c.max_len, k, (int32_t *)d_res, (float *)(d_res + off_w(nb)), stream_, err) != 0) return false;
        if ((k <= 0 || hipMemcpyAsync(ids + (size_t)c.b0 * W, d_res, (size_t)nb * W * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess) &&
            hipMemcpyAsync(weights + (size_t)c.b0 * W, d_res + off_w(nb), (size_t)nb * W * 4, hipMemcpyDeviceToHost, stream_) == hipSuccess)
            return true;
        err = "hipMemcpyAsync (results) failed";
        return false;
    }, err);
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
    Pass pass;
    pass.d_tokens = d_tokens_.as<int32_t>(); pass.d_cu = d_cu_.as<int32_t>(); pass.n_sentences = 1; pass.n_tokens = N; pass.max_len = N; pass.stream = stream_;
    pass.d_out = d_out_.as<float>();
    pass.d_hidden = d_hidden_.as<float>();
    if (eval_packed_device(pass, err) != 0) return -1;
    HIP_OK(hipStreamSynchronize(stream_), err, -1);
    if (hidden) HIP_OK(hipMemcpy(hidden, d_hidden_.p, (size_t)(L + 1) * N * H * 4, hipMemcpyDeviceToHost), err, -1);
    if (embedding) HIP_OK(hipMemcpy(embedding, d_out_.p, (size_t)H * 4, hipMemcpyDeviceToHost), err, -1);
    return 0;
}

}  // namespace bert_hip
