// index_frame.cpp — the operation frame the three indexes share (index_frame.h): stream and event, grow-only buffers, allow-lists,
// the device half of the removed-rows bitmap (the host half and the invariant: live_bits.h), remove, the merge launch and the way
// of results to the host.  The only kernel launched from here is topk_merge_kernel (search.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "index_frame.h"
#include "search_kernels.h"

namespace bert_hip {

bool IndexFrame::open(Engine *eng, const char *noun, std::string &err) {
    eng_ = eng;
    noun_ = noun;
    const bool ok = hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&busy_, hipEventDisableTiming) == hipSuccess;
    if (!ok) err = "hipStreamCreate / hipEventCreate failed";
    return ok;
}

void IndexFrame::close() {
    if (busy_) { (void)hipEventSynchronize(busy_); (void)hipEventDestroy(busy_); }
    if (stream_) { (void)hipStreamSynchronize(stream_); (void)hipStreamDestroy(stream_); }
    if (live_) (void)hipFree(live_);
    busy_ = nullptr, stream_ = nullptr, live_ = nullptr;
}

bool IndexFrame::grow(DevBuf &b, size_t bytes, std::string &err) {
    if (bytes <= b.bytes) return true;
    HIP_OK(hipEventSynchronize(busy_), err, false);          // (what is queued may still read the old buffer)
    return b.ensure(bytes, err);
}

bool IndexFrame::upload_allow(const uint32_t *allow, hipStream_t s, const uint32_t *&d_allow, std::string &err) {
    if (!allow || n_ == 0) return true;
    if (!grow(allow_, live_words(n_) * 4, err)) return false;
    HIP_OK(hipStreamWaitEvent(s, busy_, 0), err, false);
    HIP_OK(hipMemcpyAsync(allow_.p, allow, live_words(n_) * 4, hipMemcpyHostToDevice, s), err, false);
    d_allow = allow_.as<uint32_t>();
    return true;
}

// ------------------------------------------------------------------------------------------------
// removed rows
// ------------------------------------------------------------------------------------------------
bool IndexFrame::make_live(long long cap, std::string &err) {
    if (live_) return true;
    const size_t lw = live_words(cap);
    // (nothing queued, on any stream of the index, may run beside the blocking copy below)
    HIP_OK(hipEventSynchronize(busy_), err, false);
    HIP_OK(hipStreamSynchronize(stream_), err, false);
    HIP_OK(hipMalloc((void **)&live_, std::max<size_t>(lw, 1) * 4), err, false);
    bits_.make(n_, cap);
    if (lw > 0 && hipMemcpy(live_, bits_.words.data(), lw * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        drop_live();
        err = std::string("hipMemcpy (") + noun_ + " live words) failed";
        return false;
    }
    return true;
}

int IndexFrame::compact_nothing(int32_t *old_ids) {
    if (old_ids) for (int i = 0; i < n_; ++i) old_ids[i] = i;
    drop_live();
    return n_;
}

void IndexFrame::drop_live() {
    if (live_) (void)hipFree(live_);
    live_ = nullptr;
    bits_.clear();
}

bool IndexFrame::upload_live(size_t w0, size_t w1, std::string &err) {
    if (w1 <= w0) return true;
    HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, false);
    HIP_OK(hipMemcpyAsync(live_ + w0, bits_.words.data() + w0, (w1 - w0) * 4, hipMemcpyHostToDevice, stream_), err, false);
    HIP_OK(hipEventRecord(busy_, stream_), err, false);
    HIP_OK(hipStreamSynchronize(stream_), err, false);
    return true;
}

bool IndexFrame::live_for_capacity(long long cap, uint32_t *&lv, std::string &err) {
    lv = nullptr;
    if (!live_) return true;
    const size_t lw = live_words(cap), used = live_words(n_);
    const char *failed = hipMalloc((void **)&lv, lw * 4) != hipSuccess ? "hipMalloc (" : nullptr;
    if (!failed && (hipMemset(lv, 0, lw * 4) != hipSuccess || (used > 0 && hipMemcpy(lv, bits_.words.data(), used * 4, hipMemcpyHostToDevice) != hipSuccess)))
        failed = "hipMemcpy (";
    if (!failed) return true;
    (void)hipGetLastError();
    if (lv) (void)hipFree(lv);
    lv = nullptr;
    err = std::string(failed) + noun_ + " live words) failed";
    return false;
}

void IndexFrame::adopt_live(uint32_t *lv, long long cap) {
    if (!live_) return;
    (void)hipFree(live_);
    live_ = lv;
    bits_.resize(cap);
}

bool IndexFrame::install_live(const uint32_t *words, long long cap, std::string &err) {
    if (!make_live(cap, err)) return false;
    if (!bits_.install(words, n_)) { drop_live(); err = "live bits beyond the last row"; return false; }
    if (!upload_live(0, live_words(n_), err)) { drop_live(); return false; }
    return true;
}

IndexFrame::Removed IndexFrame::remove_rows(int n, const int32_t *ids, long long cap, std::vector<int32_t> &fresh, std::string &err) {
    fresh.clear();
    if (n < 0 || (n > 0 && !ids)) { err = "remove: n >= 0 and an id pointer required"; return Removed::refused; }
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= n_) { err = "remove: id " + std::to_string(ids[i]) + " is outside [0, " + std::to_string(n_) + ")"; return Removed::refused; }
    if (n == 0) return Removed::ok;
    DeviceGuard g(eng_->device());
    if (!make_live(cap, err)) return Removed::failed;
    LiveBits::Removal r = bits_.remove(ids, n);
    if (!r.ids.empty() && !upload_live(r.w0, r.w1, err)) {
        bits_.undo(r);
        return Removed::failed;
    }
    fresh = std::move(r.ids);
    return Removed::ok;
}

// ------------------------------------------------------------------------------------------------
// the merge, results to the host
// ------------------------------------------------------------------------------------------------
void IndexFrame::enqueue_merge(int nq, int n_cand, int k, int32_t *d_ids, float *d_scores, hipStream_t s) {
    MergeArgs m;
    m.ws_s = ws_s_.as<float>(); m.ws_i = ws_i_.as<int>(); m.n_cand = n_cand; m.k = k; m.L = merge_L(k); m.ids = d_ids; m.scores = d_scores;
    eng_->timed_launch("topk_merge", 0.0, s, [&] { launch_topk_merge(m, nq, s); });
}

bool IndexFrame::results_to_host(hipStream_t s, size_t at, size_t n, HostResults &r, std::string &err) {
    if (hipMemcpyAsync(r.ids.data() + at, out_ids_.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(r.scores.data() + at, out_scores_.p, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        err = "copy of the results failed";
        return false;
    }
    return true;
}

}  // namespace bert_hip
