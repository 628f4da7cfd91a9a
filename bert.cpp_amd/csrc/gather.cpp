// gather.cpp — see gather.h.
#include "gather.h"

#include <algorithm>

namespace bert_hip {

constexpr long long MIN_SHARD_TOKENS = 2048;

int eval_packed_all_devices(const Engines &engines, ShardWorkers *workers, const int32_t *tokens, const int32_t *cu, int B,
                            float *embeddings, std::string &err, float *const *d_dst, int pool_mode) {
    const int H = engines[0]->hparams().n_embd;
    int n_dev = (int)engines.size();
    const long long total = (long long)cu[B] - cu[0];
    if (!d_dst)
        while (n_dev > 1 && total < MIN_SHARD_TOKENS * n_dev) --n_dev;
    std::vector<int> bounds;
    shard_bounds(cu, B, n_dev, bounds);
    std::vector<std::string> errs((size_t)n_dev);
    auto eval = [&](int r, int b0, int b1) {
        // eval_packed_host takes the global token array and a window of the prefix sums
        return engines[r]->eval_packed_host(tokens, cu + b0, b1 - b0, embeddings ? embeddings + (size_t)b0 * H : nullptr, errs[r],
                                            d_dst ? d_dst[r] : nullptr, pool_mode);
    };
    int rc;
    if (n_dev == 1 || !workers) {
        rc = 0;
        for (int r = 0; r < n_dev && rc == 0; ++r)
            if (bounds[r + 1] > bounds[r]) rc = eval(r, bounds[r], bounds[r + 1]);
    } else {
        rc = workers->run(bounds, eval, &err);                // (a worker's exception arrives here as rc -9 + message)
    }
    if (rc != 0 && err.empty())
        for (auto &e : errs)
            if (!e.empty()) { err = e; break; }
    return rc;
}

int eval_packed_grouped_all_devices(const Engines &engines, ShardWorkers *workers, const int32_t *tokens, const int32_t *cu, int B,
                                    const int32_t *group_cu, int n_groups, float *embeddings, float *d_embeddings, std::string &err) {
    Engine &first = *engines[0];
    if (engines.size() == 1) return first.eval_packed_grouped_host(tokens, cu, B, group_cu, n_groups, embeddings, d_embeddings, err);
    // (the first engine's settings, read once: every shard and the pooling end by the same rule)
    const int pool_mode = first.options().pool_mode();
    std::vector<float> raw((size_t)B * first.hparams().n_embd);
    const int rc = eval_packed_all_devices(engines, workers, tokens, cu, B, raw.data(), err, nullptr, pool_mode | POOL_RAW);
    if (rc != 0) return rc;
    return first.eval_packed_grouped_host(tokens, cu, B, group_cu, n_groups, embeddings, d_embeddings, err, raw.data(), pool_mode);
}

void gather_runs(const int32_t *cu, int n_sentences, long long tokens_per_run, std::vector<int> &runs) {
    runs.assign(1, 0);
    for (int b = 1; b <= n_sentences; ++b)
        if (b == n_sentences || (long long)cu[b + 1] - cu[runs.back()] > tokens_per_run) runs.push_back(b);
}

EmbeddingGather::~EmbeddingGather() {
    for (size_t d = 0; d < xstream_.size(); ++d) {
        if (d < devs_.size()) (void)hipSetDevice(devs_[d]);
        if (xstream_[d]) { (void)hipStreamSynchronize(xstream_[d]); (void)hipStreamDestroy(xstream_[d]); }
    }
    for (hipEvent_t e : xdone_) if (e) (void)hipEventDestroy(e);
}

void EmbeddingGather::drain(const Engines &engines) {
    for (int d = 0; d < (int)engines.size(); ++d) {
        if (hipSetDevice(engines[d]->device()) != hipSuccess) continue;
        (void)hipStreamSynchronize(engines[d]->stream());
        if (d < (int)xstream_.size() && xstream_[d]) (void)hipStreamSynchronize(xstream_[d]);
    }
}

bool EmbeddingGather::run(const Engines &engines, ShardWorkers *workers, const int32_t *tokens, const int32_t *cu, int n_sentences,
                          float **d_embeddings, std::string &err) {
    const int n_dev = (int)engines.size(), H = engines[0]->hparams().n_embd;
    const bool exchange = n_dev > 1 || rccl_single;
    bool issued = false;
    auto fail = [&](const std::string &what) {
        err = what;
        if (issued) drain(engines);
        return false;
    };
    if (shard_out_.empty())
        for (int d = 0; d < 2 * n_dev; ++d) { shard_out_.emplace_back(new DevBuf); if (d < n_dev) gathered_.emplace_back(new DevBuf); }
    // every run of about `super` tokens per device is sharded over the devices by token count like a call of its own, and its
    // exchange is issued on the devices' EXCHANGE streams as soon as its shards are computed — it runs under the next run's
    // compute.  Rows land at their global positions, so the result does not depend on the cut.  A call that fits one run is
    // one shard per device and one exchange.
    const long long super = super_tokens > 0 ? super_tokens : 4ll * 262144;
    std::vector<int> runs{0, n_sentences};
    if (exchange) gather_runs(cu, n_sentences, super * n_dev, runs);
    const int n_runs = (int)runs.size() - 1;
    devs_.clear();
    for (auto &e : engines) devs_.push_back(e->device());
    size_t max_rows = 1;
    std::vector<std::vector<int>> run_bounds((size_t)n_runs);
    for (int k = 0; k < n_runs; ++k) {
        shard_bounds(cu + runs[k], runs[k + 1] - runs[k], n_dev, run_bounds[k]);
        for (int d = 0; d < n_dev; ++d) max_rows = std::max(max_rows, (size_t)(run_bounds[k][d + 1] - run_bounds[k][d]));
    }
    if (exchange && (int)xstream_.size() < n_dev) { xstream_.resize(n_dev, nullptr); xdone_.resize(2 * n_dev, nullptr); }
    std::vector<float *> dst((size_t)n_dev);
    for (int d = 0; d < n_dev; ++d) {
        if (hipSetDevice(devs_[d]) != hipSuccess) return fail("hipSetDevice failed");
        for (int sl = 0; sl < (n_runs > 1 ? 2 : 1); ++sl)
            if (!shard_out_[2 * d + sl]->ensure(max_rows * H * 4, err)) return fail(err);
        if (exchange && !gathered_[d]->ensure((size_t)n_sentences * H * 4, err)) return fail(err);
        // (no exchange: the one device's shard buffer IS the result)
        dst[d] = exchange ? gathered_[d]->as<float>() : shard_out_[2 * d]->as<float>();
        if (exchange) {
            if (!xstream_[d] && hipStreamCreateWithFlags(&xstream_[d], hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
            for (int sl = 0; sl < 2; ++sl)
                if (!xdone_[2 * d + sl] && hipEventCreateWithFlags(&xdone_[2 * d + sl], hipEventDisableTiming) != hipSuccess) return fail("hipEventCreate failed");
        }
    }
    if (exchange && !rccl.init(devs_, err)) return fail(err);
    const bool threaded = exchange && workers && workers->n_threads() == n_dev - 1;
    for (int k = 0; k < n_runs; ++k) {
        const int sl = k & 1, b0 = runs[k], nb = runs[k + 1] - b0;
        std::vector<float *> src((size_t)n_dev);
        for (int d = 0; d < n_dev; ++d) {
            src[d] = shard_out_[2 * d + sl]->as<float>();
            // the exchange of run k - 2 read this buffer
            if (exchange && k >= 2 && (hipSetDevice(devs_[d]) != hipSuccess || hipEventSynchronize(xdone_[2 * d + sl]) != hipSuccess))
                return fail("waiting for an exchange failed");
        }
        // (blocking: the shards are complete in src when this returns)
        if (eval_packed_all_devices(engines, workers, tokens, cu + b0, nb, nullptr, err, src.data()) != 0) return fail(err);
        if (!exchange) break;
        // this run's exchange step (RCCL over xGMI): every device receives every other device's shard of the run, at rows
        // b0 + bounds of its matrix; not waited for here
        const std::vector<int> &bounds = run_bounds[k];
        bool ok;
        if (threaded) {
            // every device's call from the host thread that serves the device (worker d - 1, the caller for device 0)
            std::vector<std::string> errs((size_t)n_dev);
            const int rc = workers->run_each(n_dev, [&](int d) {
                return rccl.exchange_on(d, src[d], dst[d] + (size_t)b0 * H, bounds, H, xstream_[d], errs[d]) ? 0 : -3; }, &err);
            for (auto &e : errs) if (err.empty() && !e.empty()) err = e;
            ok = rc == 0;
        } else {
            std::vector<float *> at((size_t)n_dev);
            for (int d = 0; d < n_dev; ++d) at[d] = dst[d] + (size_t)b0 * H;
            ok = rccl.all_gather(src.data(), at.data(), bounds, H, xstream_.data(), err);
        }
        issued = true;                                    // (even a failed attempt may have queued part of the step)
        if (!ok) return fail(err);
        for (int d = 0; d < n_dev; ++d)
            if (hipSetDevice(devs_[d]) != hipSuccess || hipEventRecord(xdone_[2 * d + sl], xstream_[d]) != hipSuccess) return fail("hipEventRecord failed");
    }
    for (int d = 0; d < n_dev; ++d) {
        if (hipSetDevice(devs_[d]) != hipSuccess || hipStreamSynchronize(engines[d]->stream()) != hipSuccess ||
            (exchange && hipStreamSynchronize(xstream_[d]) != hipSuccess))
            return fail("synchronisation failed");
        d_embeddings[d] = dst[d];
    }
    return true;
}

}  // namespace bert_hip
