// live_bits.h — the removed-rows bitmap of the three indexes (search.h, sparse_index.h, token_index.h), host half: one bit per row
// or document (set = live) in 32-bit words, and the count of removed ones.  No device code: index_frame.h keeps the device words in
// step with it, and tools/live_bits_cases.cpp checks it against a plain model on the CPU.
//
// THE INVARIANT, stated here and referred to elsewhere: the mirror is as long as the index's capacity (live_words(cap) words), and its
// bits at and beyond the index's size are zero.  The device words have the same length; their bits at and beyond size are whatever
// they were (a search ignores them, and the add that reuses those rows sets them).  A file holds the first live_words(size) words.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bert_hip {

// the words that `rows` rows take
inline size_t live_words(long long rows) { return (size_t)((rows + 31) / 32); }

// bits of rows [first, first + n) := 1 in a host copy of the words
inline void live_set_range_host(std::vector<uint32_t> &live, int first, int n) {
    for (long long r = first; r < (long long)first + n;) {
        const size_t w = (size_t)(r >> 5);
        const int b = (int)(r & 31), c = (int)std::min<long long>(32 - b, (long long)first + n - r);
        live[w] |= (c == 32 ? ~0u : ((1u << c) - 1u) << b);
        r += c;
    }
}

// no bit at or beyond row n in `last`, the word that holds row n - 1 (the one check of "live bits beyond the last row")
inline bool live_tail_clear(uint32_t last, long long n) { return (n & 31) == 0 || (last >> (n & 31)) == 0; }

struct LiveBits {
    std::vector<uint32_t> words;
    int n_removed = 0;

    bool test(long long r) const { return words[(size_t)(r >> 5)] >> (r & 31) & 1u; }
    // every one of n rows live, in a mirror for `cap` rows
    void make(int n, long long cap) {
        words.assign(live_words(cap), 0u);
        if (n > 0) live_set_range_host(words, 0, n);
        n_removed = 0;
    }
    void clear() { words.clear(); n_removed = 0; }
    // a new capacity, the bits kept
    void resize(long long cap) { words.resize(live_words(cap), 0u); }
    void set_range(int first, int n) { live_set_range_host(words, first, n); }

    // What one remove() changed: the ids it newly removed, in the caller's order (repeats and removed rows left out), and the words
    // it touched, [w0, w1) — empty if it removed nothing
    struct Removal {
        std::vector<int32_t> ids;
        size_t w0 = SIZE_MAX, w1 = 0;
    };
    // ids [n], each in [0, size): the caller checks
    Removal remove(const int32_t *ids, int n) {
        Removal r;
        for (int i = 0; i < n; ++i) {
            const size_t w = (size_t)ids[i] >> 5;
            const uint32_t bit = 1u << (ids[i] & 31);
            if (!(words[w] & bit)) continue;
            words[w] &= ~bit;
            r.ids.push_back(ids[i]);
            r.w0 = std::min(r.w0, w);
            r.w1 = std::max(r.w1, w + 1);
        }
        n_removed += (int)r.ids.size();
        return r;
    }
    // the mirror as it was before that remove
    void undo(const Removal &r) {
        for (int32_t id : r.ids) words[(size_t)id >> 5] |= 1u << (id & 31);
        n_removed -= (int)r.ids.size();
    }

    // The index shrinks from old_n to new_n rows: the dropped rows' bits := 0.  Those of them that were removed no longer count;
    // was_removed(id) is called for each, ascending.  Returns how many they were
    template <class F> int truncate(int old_n, int new_n, F &&was_removed) {
        int dropped = 0;
        for (int r = new_n; r < old_n; ++r) {
            if (!test(r)) { ++dropped; was_removed(r); }
            words[(size_t)r >> 5] &= ~(1u << (r & 31));
        }
        n_removed -= dropped;
        return dropped;
    }
    int truncate(int old_n, int new_n) { return truncate(old_n, new_n, [](int) {}); }

    // the live ones of n rows, ascending: the former id of each row that a compaction keeps
    std::vector<int32_t> kept(int n) const {
        std::vector<int32_t> map;
        map.reserve((size_t)(n - n_removed));
        for (int r = 0; r < n; ++r)
            if (test(r)) map.push_back(r);
        return map;
    }

    // The first live_words(n) words := w, as a file holds them for an index of n rows; the mirror is already made for the capacity.
    // false, and nothing changed, if w has a bit at or beyond row n
    bool install(const uint32_t *w, int n) {
        const size_t nw = live_words(n);
        if (nw > 0 && !live_tail_clear(w[nw - 1], n)) return false;
        std::copy(w, w + nw, words.begin());
        n_removed = n;
        for (size_t i = 0; i < nw; ++i) n_removed -= __builtin_popcount(w[i]);
        return true;
    }
};

}  // namespace bert_hip
