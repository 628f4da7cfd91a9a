// live_bits_cases — live_bits.h's removed-rows bitmap on its own, for a sanitizer build on the CPU: every operation the three indexes
// perform on their host mirror, each compared with a plain std::vector<bool> model kept alongside, at the sizes around a word edge
// and around the first capacity step.
//   make -C bert.cpp_amd check-host
#include <algorithm>
#include <cstdio>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "live_bits.h"

using namespace bert_hip;

namespace {

int failures = 0;

void report(const std::string &name, bool ok) {
    printf("%-4s %s\n", ok ? "ok" : "FAIL", name.c_str());
    failures += !ok;
}

const int SIZES[] = {0, 1, 31, 32, 33, 63, 64, 65, 1024, 1025};
// the capacity an index of n rows has: the first step is 1024, then half as much again
long long cap_of(int n) { return n <= 1024 ? 1024 : 1536; }

// the bitmap and its model: model[r] = row r is live, for the n rows of the index
struct Pair {
    LiveBits b;
    std::vector<bool> model;
    long long cap = 0;
    Pair(int n, long long c) : model((size_t)n, true), cap(c) { b.make(n, c); }
    int n() const { return (int)model.size(); }

    // the invariant and the model: as long as the capacity, bit r = model[r] below size, zero at and beyond it, the count
    bool agree() const {
        if (b.words.size() != live_words(cap)) return false;
        int removed = 0;
        for (size_t r = 0; r < b.words.size() * 32; ++r) {
            const bool want = r < model.size() && model[r];
            if (b.test((long long)r) != want) return false;
            removed += r < model.size() && !model[r];
        }
        return b.n_removed == removed;
    }
    // remove(ids) on both; checks the returned list, the dirty range and the count against the model
    bool remove(const std::vector<int32_t> &ids, LiveBits::Removal *out = nullptr) {
        std::vector<int32_t> want;
        size_t w0 = SIZE_MAX, w1 = 0;
        for (int32_t id : ids)
            if (model[(size_t)id]) {
                model[(size_t)id] = false;
                want.push_back(id);
                w0 = std::min(w0, (size_t)id / 32);
                w1 = std::max(w1, (size_t)id / 32 + 1);
            }
        // (a heap copy of exactly the ids: the sanitizer sees a read beyond them)
        std::unique_ptr<int32_t[]> p(new int32_t[ids.size() ? ids.size() : 1]);
        std::copy(ids.begin(), ids.end(), p.get());
        const LiveBits::Removal r = b.remove(p.get(), (int)ids.size());
        if (out) *out = r;
        return r.ids == want && (want.empty() ? r.w1 <= r.w0 : (r.w0 == w0 && r.w1 == w1)) && agree();
    }
    // truncate on both; checks the reported "already removed among the dropped" (their ids, ascending, and their number)
    bool truncate(int new_n) {
        std::vector<int> want, got;
        for (int r = new_n; r < n(); ++r)
            if (!model[(size_t)r]) want.push_back(r);
        const int cnt = b.truncate(n(), new_n, [&](int r) { got.push_back(r); });
        model.resize((size_t)new_n);
        return got == want && cnt == (int)want.size() && agree();
    }
    // an add of m rows: they are live, and take the ids behind the last
    bool add(int m) {
        b.set_range(n(), m);
        model.resize(model.size() + (size_t)m, true);
        return agree();
    }
    bool kept() const {
        std::vector<int32_t> want;
        for (int r = 0; r < n(); ++r)
            if (model[(size_t)r]) want.push_back(r);
        return b.kept(n()) == want;
    }
};

std::vector<int32_t> iota(int first, int count) {
    std::vector<int32_t> v((size_t)count);
    std::iota(v.begin(), v.end(), first);
    return v;
}

void cases_of_size(int n) {
    const std::string at = " at " + std::to_string(n);
    report("all live, kept ids" + at, Pair(n, cap_of(n)).agree() && Pair(n, cap_of(n)).kept());
    if (n == 0) {
        Pair p(0, cap_of(0));
        LiveBits::Removal r;
        report("remove nothing" + at, p.remove({}, &r) && r.ids.empty());
        return;
    }
    { Pair p(n, cap_of(n)); report("remove the first row" + at, p.remove({0}) && p.kept()); }
    { Pair p(n, cap_of(n)); report("remove the last row" + at, p.remove({n - 1}) && p.kept()); }
    if (n >= 32) {
        Pair p(n, cap_of(n));
        const int w = (n - 32) / 32;                         // the last whole word
        report("remove a whole word" + at, p.remove(iota(32 * w, 32)) && p.b.words[(size_t)w] == 0u && p.kept());
    }
    { Pair p(n, cap_of(n)); report("remove every row" + at, p.remove(iota(0, n)) && p.b.n_removed == n && p.b.kept(n).empty()); }
    {
        Pair p(n, cap_of(n));
        LiveBits::Removal r;
        const bool ok = p.remove({n - 1, 0, n - 1, 0, n / 2}, &r);        // repeats inside one call
        report("remove with repeats" + at, ok && (int)r.ids.size() == p.b.n_removed);
        report("remove an already removed id" + at, p.remove({n / 2}, &r) && r.ids.empty() && r.w1 <= r.w0);
    }
    {
        Pair p(n, cap_of(n));
        p.remove({n / 3});
        const std::vector<uint32_t> before = p.b.words;
        const int removed = p.b.n_removed;
        const LiveBits::Removal r = p.b.remove(iota(0, n).data(), n);
        p.b.undo(r);
        report("undo restores the words and the count" + at, p.b.words == before && p.b.n_removed == removed && p.agree());
    }
    {
        // resize to the next capacity keeps the bits and zero-fills the rest
        Pair p(n, cap_of(n));
        p.remove({0, n - 1});
        p.cap = p.cap * 3 / 2;
        p.b.resize(p.cap);
        report("resize to a larger capacity" + at, p.agree() && p.add(p.cap - n > 40 ? 40 : (int)(p.cap - n)) && p.kept());
    }
    // truncate from this size to every smaller one of the list
    for (int m : SIZES) {
        if (m >= n) continue;
        Pair p(n, cap_of(n));
        std::vector<int32_t> ids = {0, n - 1, m, std::max(m - 1, 0), (m + n) / 2};
        p.remove(ids);
        bool ok = p.truncate(m);
        // set-range across a word edge after the truncate: the add reuses the dropped ids, and they are live again
        ok = ok && p.add(std::min(n - m, 34)) && p.kept();
        report("truncate to " + std::to_string(m) + ", then add" + at, ok);
    }
}

void install_cases(int n) {
    const std::string at = " at " + std::to_string(n);
    Pair p(n, cap_of(n));
    for (int r = 0; r < n; r += 3) p.model[(size_t)r] = false;
    const size_t nw = live_words(n);
    // (a heap copy of exactly the file's words)
    std::unique_ptr<uint32_t[]> w(new uint32_t[nw ? nw : 1]);
    std::fill(w.get(), w.get() + nw, 0u);
    for (int r = 0; r < n; ++r)
        if (p.model[(size_t)r]) w[(size_t)r / 32] |= 1u << (r % 32);
    report("install accepts and counts" + at, p.b.install(w.get(), n) && p.agree() && p.kept());
    if (n % 32 == 0) return;
    // a stray bit in the last word, at every place beyond the last row
    bool all = true;
    for (int bit = n % 32; bit < 32; ++bit) {
        Pair q(n, cap_of(n));
        w[nw - 1] |= 1u << bit;
        all = all && !q.b.install(w.get(), n) && q.agree();                 // refused, and nothing changed
        all = all && !live_tail_clear(w[nw - 1], n);
        w[nw - 1] &= ~(1u << bit);
    }
    report("install rejects a stray bit beyond the last row" + at, all);
}

}  // namespace

int main() {
    for (int n : SIZES) cases_of_size(n);
    for (int n = 0; n <= 97; ++n) install_cases(n);        // every n & 31, through three words
    for (int n : {1024, 1025}) install_cases(n);
    {
        // the capacity step itself: 1024 rows in a mirror for 1024, three removed, grown to 1536, 100 rows added
        Pair p(1024, 1024);
        bool ok = p.remove({0, 31, 1023});
        p.cap = 1536;
        p.b.resize(p.cap);
        ok = ok && p.agree() && p.add(100) && p.kept() && p.n() == 1124 && p.b.n_removed == 3;
        report("1024 -> 1536 with removed rows, then 100 added", ok);
    }
    report("live_words", live_words(0) == 0 && live_words(1) == 1 && live_words(32) == 1 && live_words(33) == 2 && live_words(0x7fffffffLL) == (1u << 26));
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
