// index_frame.h — what the embedding index (search.h), the sparse index (sparse_index.h) and the token index (token_index.h) have in
// common whatever a row looks like (index_frame.cpp): the engine, the stream of the host routes and the one event, buffers that only
// grow, a caller's allow-list on its way to the device, the device words of the removed-rows bitmap beside their host mirror
// (live_bits.h, which states the invariant), remove(), the merge of per-slice lists and the way of results back to the host.  Each
// index derives from it and keeps its own storage, capacity rule, checks and return codes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "engine.h"
#include "live_bits.h"

namespace bert_hip {

// an index's device for the length of a call
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(d);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// the results of a blocking route, [n] ids and scores, gathered on the host: the caller's arrays are written only on success
struct HostResults {
    std::vector<int32_t> ids;
    std::vector<float> scores;
    explicit HostResults(size_t n) : ids(n), scores(n) {}
    void deliver(int32_t *i, float *s) const { memcpy(i, ids.data(), ids.size() * 4); memcpy(s, scores.data(), scores.size() * 4); }
};

class IndexFrame {
protected:
    IndexFrame() = default;
    ~IndexFrame() { close(); }

    // the engine, the stream and the event; noun ("index", "sparse index", "token index") names the index in device errors
    bool open(Engine *eng, const char *noun, std::string &err);
    // waits for the event, then for the stream, and destroys both; the bitmap goes too.  First thing in a destructor, under its
    // DeviceGuard: the index's own storage is freed behind it
    void close();

    // b of at least `bytes` (what is queued may still read the old buffer: behind the event)
    bool grow(DevBuf &b, size_t bytes, std::string &err);
    // a host allow-list (null, or an empty index: d_allow stays null) into allow_, on s behind whatever is queued on the index; the
    // searches that read it follow on s
    bool upload_allow(const uint32_t *allow, hipStream_t s, const uint32_t *&d_allow, std::string &err);

    // Removed rows.  make_live: the bitmap of an index that had none, every row live, for `cap` rows (no-op if there is one); blocking
    bool make_live(long long cap, std::string &err);
    void drop_live();
    // compact() of an index without removed rows: every row keeps its id, the bitmap (if any) goes; the size
    int compact_nothing(int32_t *old_ids);
    // mirror words [w0, w1) -> device, on the index's stream behind whatever is queued; blocking
    bool upload_live(size_t w0, size_t w1, std::string &err);
    // Growth to `cap` rows in two steps, so that the index can make all its new storage before it lets any old go: the new device
    // words (zero beyond the mirror's live_words(n_)); then, nothing having failed, they replace the old and the mirror follows
    bool live_for_capacity(long long cap, uint32_t *&lv, std::string &err);
    void adopt_live(uint32_t *lv, long long cap);
    // the file's words of a loaded index of n_ rows become its bitmap (already checked: live_tail_clear); blocking
    bool install_live(const uint32_t *words, long long cap, std::string &err);
    // remove() of all three: ids [n] marked removed, `fresh` the ones newly so.  refused: an argument, nothing changed; failed: the
    // device, the mirror as it was.  A message in err either way; the index maps the outcome to its own return code
    enum class Removed { ok, refused, failed };
    Removed remove_rows(int n, const int32_t *ids, long long cap, std::vector<int32_t> &fresh, std::string &err);

    // topk_merge over ws_s_ / ws_i_ [nq][n_cand] -> d_ids / d_scores [nq][k], on s
    void enqueue_merge(int nq, int n_cand, int k, int32_t *d_ids, float *d_scores, hipStream_t s);
    // out_ids_ / out_scores_ [n] -> r at entry `at`, on s behind what it holds; blocking (a failure leaves s synchronised)
    bool results_to_host(hipStream_t s, size_t at, size_t n, HostResults &r, std::string &err);

    Engine *eng_ = nullptr;
    int n_ = 0;                                         // rows or documents
    // removed rows: the device words and their host mirror (live_bits.h), both absent until the first remove
    uint32_t *live_ = nullptr;
    LiveBits bits_;
    DevBuf ws_s_, ws_i_;                                // per-(query, slice) lists, or a rescore's scores and ids
    DevBuf out_ids_, out_scores_;                       // host routes: results
    DevBuf allow_;                                      // host routes: the caller's allow-list on the device
    hipStream_t stream_ = nullptr;                      // the host routes' stream
    // the index's buffers serve ONE operation at a time: each waits (on its own stream) for the previous one's event
    hipEvent_t busy_ = nullptr;

private:
    const char *noun_ = "index";
};

}  // namespace bert_hip
