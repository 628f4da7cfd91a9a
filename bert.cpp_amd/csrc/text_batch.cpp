// text_batch.cpp — see text_batch.h.  Reference behaviour mirrored here: bert_encode_batch, reference bert.cpp:952-1022 (it sorts
// by length and loops with batch size 1; per-sentence results do not depend on batching).
#include "text_batch.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <deque>
#include <exception>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>

namespace bert_hip {

void TextBatcher::tokenize_many(int32_t n_threads, int32_t n_inputs, const char **texts, int32_t *tokens, int32_t *n_tokens) {
    const int32_t N = n_max_tokens;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    int nt = std::min<int>({n_threads > 0 ? n_threads : 1, (int)hw, (n_inputs + 31) / 32});
    if (nt <= 1) {
        for (int32_t i = 0; i < n_inputs; ++i) tok->tokenize(texts[i], tokens + (size_t)i * N, &n_tokens[i], N);
        return;
    }
    std::atomic<int32_t> next{0};
    auto work = [&](int) {
        for (;;) {
            const int32_t i0 = next.fetch_add(16);
            if (i0 >= n_inputs) break;
            const int32_t i1 = std::min(n_inputs, i0 + 16);
            for (int32_t i = i0; i < i1; ++i) tok->tokenize(texts[i], tokens + (size_t)i * N, &n_tokens[i], N);
        }
        return 0;
    };
    // persistent workers (a thread that could not be started is not an error: the others, at least the caller, take its share)
    // (rebuilt only when MORE threads are asked for than were ever asked for: a pool that came up short — a thread that could
    // not be started — is kept, not torn down and recreated on every call)
    if (!workers || workers_asked < nt - 1) { workers.reset(new ShardWorkers(nt - 1)); workers_asked = nt - 1; }
    std::string err;
    if (workers->run_each(nt, work, &err) != 0) throw std::runtime_error("tokenizer worker: " + err);
}

void TokenGroup::pack(int32_t N, int32_t n) {
    cu.resize((size_t)n + 1);
    cu[0] = 0;
    n_ok = n;
    for (int32_t i = 0; i < n; ++i) {
        if (n_tokens[i] <= 0 || n_tokens[i] > N) { n_ok = i; break; }
        cu[i + 1] = cu[i] + n_tokens[i];
    }
    const size_t T = (size_t)cu[n_ok];
    if (packed_cap < T) { packed.reset(new int32_t[T + T / 4]); packed_cap = T + T / 4; }
    for (int32_t i = 0; i < n_ok; ++i) memcpy(packed.get() + cu[i], ids.get() + (size_t)i * N, sizeof(int32_t) * n_tokens[i]);
}

void TokenGroup::tokenize(TextBatcher &tb, int32_t n_threads, int32_t n, const char **texts) {
    const size_t need = (size_t)tb.n_max_tokens * n;
    if (ids_cap < need) { ids.reset(new int32_t[need]); ids_cap = need; }
    n_tokens.resize(n);
    tb.tokenize_many(n_threads, n, texts, ids.get(), n_tokens.data());
    pack(tb.n_max_tokens, n);
}

int32_t encode_group_size(int k, int32_t left) {
    const int32_t g = (int32_t)(2048 << std::min(k, 3));
    return left - g < g / 4 ? left : g;
}

int32_t TextBatcher::encode_groups(int32_t n_threads, int32_t n_inputs, const char **texts, const EvalGroup &eval) {
#ifdef BERT_HIP_HOST_TRACE
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
#endif
    group[0].tokenize(*this, n_threads, encode_group_size(0, n_inputs), texts);
#ifdef BERT_HIP_HOST_TRACE
    fprintf(stderr, "[encode] first group tokenized in %.3f ms\n", now() - t_begin);
#endif
    int32_t total = 0;
    for (int32_t i0 = 0, k = 0; i0 < n_inputs; ++k) {
        const int32_t n = encode_group_size(k, n_inputs - i0), n_next = n_inputs - i0 - n > 0 ? encode_group_size(k + 1, n_inputs - i0 - n) : 0;
        std::thread ahead;
        std::exception_ptr ahead_error;
        if (n_next > 0) {
            auto job = [&, k, i0, n, n_next] {
                try { group[(k + 1) & 1].tokenize(*this, n_threads, n_next, texts + i0 + n); } catch (...) { ahead_error = std::current_exception(); }
            };
            try { ahead = std::thread(job); } catch (const std::system_error &) { job(); }     // no thread: tokenize in line
        }
        int32_t done = -1;
        std::exception_ptr eval_error;
#ifdef BERT_HIP_HOST_TRACE
        const double t_e0 = now();
#endif
        try {
            const TokenGroup &g = group[k & 1];
            if (g.n_ok < n) fprintf(stderr, "bert_encode_batch: input %d cannot be evaluated (%d tokens)\n", i0 + g.n_ok, g.n_tokens[g.n_ok]);
            done = g.n_ok > 0 ? eval(g, i0) : 0;
        } catch (...) { eval_error = std::current_exception(); }
#ifdef BERT_HIP_HOST_TRACE
        const double t_e1 = now();
#endif
        if (ahead.joinable()) ahead.join();                   // never leave the scope with a running thread
#ifdef BERT_HIP_HOST_TRACE
        fprintf(stderr, "[encode] group %d: %d texts, eval %.3f ms, then waited %.3f ms for the tokenizer\n", k, n, t_e1 - t_e0, now() - t_e1);
#endif
        if (eval_error) std::rethrow_exception(eval_error);
        if (ahead_error) std::rethrow_exception(ahead_error);
        total += done > 0 ? done : 0;
        if (done != n) break;                                 // outputs after the failure stay untouched
        i0 += n;
    }
    return total;
}

void TextBatcher::tokenize_long(const char *text, std::vector<int32_t> &ids) const {
    const size_t b = strlen(text);
    if (b > (size_t)INT32_MAX - 2) throw std::length_error("text too long to tokenize");
    ids.resize(b + 2);
    int32_t n = 0;
    tok->tokenize(text, ids.data(), &n, (int32_t)(b + 2));
    ids.resize((size_t)n);
}

int32_t LongGroup::append(const std::vector<int32_t> &ids, int32_t window, int32_t stride) {
    const int32_t n = (int32_t)ids.size(), count = plan_windows(n, window, stride, nullptr, 0);
    if (count == 1) {
        packed.insert(packed.end(), ids.begin(), ids.end());
        cu.push_back((int32_t)packed.size());
    } else {
        std::vector<int32_t> starts((size_t)count);
        plan_windows(n, window, stride, starts.data(), count);
        for (int32_t i = 0; i < count; ++i) {
            packed.push_back(ids.front());
            packed.insert(packed.end(), ids.begin() + 1 + starts[i], ids.begin() + 1 + starts[i] + (window - 2));
            packed.push_back(ids.back());
            cu.push_back((int32_t)packed.size());
        }
    }
    group_cu.push_back((int32_t)cu.size() - 1);
    return count;
}

int32_t TextBatcher::encode_long_groups(int32_t n_threads, int32_t n_inputs, const char **texts, int32_t window, int32_t stride,
                                        int32_t *n_windows, const EvalLongGroup &eval) {
    constexpr int32_t SLAB = 256;                             // texts tokenized at a time (about a quarter of a group at 1000 tokens a text and window 128)
    std::deque<std::vector<int32_t>> pending;                 // texts next_build .. next_tok - 1, tokenized and not yet in a group
    std::vector<std::vector<int32_t>> slab;
    int32_t next_tok = 0, next_build = 0;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    auto tokenize_slab = [&]() {
        const int32_t c = std::min(SLAB, n_inputs - next_tok);
        const char **t = texts + next_tok;
        slab.resize((size_t)c);
        const int nt = std::min<int>({n_threads > 0 ? n_threads : 1, (int)hw, (int)c});
        if (nt <= 1) {
            for (int32_t i = 0; i < c; ++i) tokenize_long(t[i], slab[i]);
        } else {
            std::atomic<int32_t> next{0};
            auto work = [&](int) {
                for (int32_t i; (i = next.fetch_add(1)) < c;) tokenize_long(t[i], slab[i]);
                return 0;
            };
            if (!workers || workers_asked < nt - 1) { workers.reset(new ShardWorkers(nt - 1)); workers_asked = nt - 1; }
            std::string err;
            if (workers->run_each(nt, work, &err) != 0) throw std::runtime_error("tokenizer worker: " + err);
        }
        for (auto &ids : slab) pending.push_back(std::move(ids));
        next_tok += c;
    };
    LongGroup &g = long_group;
    while (next_build < n_inputs) {
        const int32_t i0 = next_build;
        g.clear();
        for (;;) {
            if (pending.empty()) {
                if (next_tok == n_inputs) break;
                tokenize_slab();
            }
            const std::vector<int32_t> &ids = pending.front();
            const int32_t count = plan_windows((int32_t)ids.size(), window, stride, nullptr, 0);
            if (g.n_texts() > 0 && (int64_t)g.n_windows() + count > LONG_GROUP_WINDOWS) break;
            // (the ids of a group are counted in int32, like every packed batch)
            if ((int64_t)g.packed.size() + (int64_t)count * window > INT32_MAX) {
                if (g.n_texts() > 0) break;
                throw std::length_error("a text's windows hold more than 2^31 ids");
            }
            g.append(ids, window, stride);
            pending.pop_front();
            ++next_build;
        }
        if (eval(g, i0) != g.n_texts()) return i0;
        if (n_windows)
            for (int32_t i = 0; i < g.n_texts(); ++i) n_windows[i0 + i] = g.group_cu[i + 1] - g.group_cu[i];
    }
    return n_inputs;
}

}  // namespace bert_hip
