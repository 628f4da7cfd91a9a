// sparse_index.cpp — the host side of the sparse index (sparse_index.h): storage and its growth, add, the search and its chunks,
// rescoring, reading rows back, the checks of the host forms, compaction and the file form (live bits, remove, stream and event:
// index_frame.h; file frame: index_io.h).  Kernels: sparse_index.hip behind sparse_index_kernels.h (the merge: search.hip).  The postings and the launches of the inverted search are sparse_postings.cpp; the
// searches here take `inverted` and share their checks, chunking and copies with it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include <sys/types.h>

#include "index_io.h"
#include "search_kernels.h"
#include "sparse_index.h"

namespace bert_hip {

namespace {

int blocks_of(long long rows) { return (int)((rows + SPARSE_BLOCK_ROWS - 1) / SPARSE_BLOCK_ROWS); }
// the most workspace entries (nq' * slices * k) a chunk of up to nqc queries takes: the slice count falls as the tiles grow
size_t ws_entries_bound(int dtype, int n_vocab, int n_rows, int nqc, int k, int qb_pref) {
    size_t ent = 0;
    SparseScanGeometry g;
    for (int q = 1; q <= nqc; ++q)
        if (sparse_scan_geometry(dtype, n_vocab, n_rows, q, k, g, qb_pref)) ent = std::max(ent, (size_t)q * g.max_slices * k);
    return ent;
}

// Host rows or queries [n][kk]: every id in [-1, n_vocab), none twice in an entry, every used weight finite — as f16 where the
// index stores f16 (as_f16).  false + err names the first offender.
bool check_terms(const char *what, int n, int kk, const int32_t *ids, const float *w, int n_vocab, bool as_f16, std::string &err) {
    std::vector<int32_t> seen;
    for (int i = 0; i < n; ++i) {
        seen.clear();
        for (int j = 0; j < kk; ++j) {
            const int32_t id = ids[(size_t)i * kk + j];
            if (id == -1) continue;
            if (id < -1 || id >= n_vocab) { err = std::string(what) + " " + std::to_string(i) + ": id " + std::to_string(id) + " outside [-1, " + std::to_string(n_vocab) + ")"; return false; }
            const float x = w[(size_t)i * kk + j];
            if (!std::isfinite(as_f16 ? (float)(half_t)x : x)) { err = std::string(what) + " " + std::to_string(i) + ": the weight of id " + std::to_string(id) + " is not finite" + (as_f16 ? " as f16" : ""); return false; }
            seen.push_back(id);
        }
        std::sort(seen.begin(), seen.end());
        const auto dup = std::adjacent_find(seen.begin(), seen.end());
        if (dup != seen.end()) { err = std::string(what) + " " + std::to_string(i) + ": id " + std::to_string(*dup) + " appears twice"; return false; }
    }
    return true;
}

// 1 = go on, 0 = nothing to do, -2 = refused
int check_add(int n, int k_in, const void *ids, const void *w, int width, int size, std::string &err) {
    if (k_in < 1 || k_in > width) { err = "add: 1 <= k_in <= width (" + std::to_string(width) + ") required"; return -2; }
    if (n < 0 || (n > 0 && (!ids || !w))) { err = "add: n >= 0 and id / weight pointers required"; return -2; }
    if ((long long)size + n > INT_MAX - SPARSE_BLOCK_ROWS) { err = "add: an index holds at most 2^31 - 65 rows"; return -2; }
    return n > 0;
}

int check_search(int nq, int kq, const void *qi, const void *qw, int k, const void *ids, const void *scores, std::string &err) {
    if (k < 1 || k > SparseIndex::MAX_K) { err = "search: k must be 1 .. 256"; return -2; }
    if (kq < 1 || kq > SparseIndex::MAX_TERMS) { err = "search: kq must be 1 .. 256"; return -2; }
    if (nq < 0 || (nq > 0 && (!qi || !qw || !ids || !scores))) { err = "search: n_queries >= 0 and query / result pointers required"; return -2; }
    return nq > 0;
}

int check_rescore(int nq, int kq, const void *qi, const void *qw, int n_cand, const void *cand, int k, const void *ids, const void *scores, std::string &err) {
    if (k < 1 || k > SparseIndex::MAX_K) { err = "rescore: k must be 1 .. 256"; return -2; }
    if (kq < 1 || kq > SparseIndex::MAX_TERMS) { err = "rescore: kq must be 1 .. 256"; return -2; }
    if (n_cand < 1 || n_cand > SparseIndex::MAX_CAND) { err = "rescore: n_cand must be 1 .. 1024"; return -2; }
    if (nq < 0 || (nq > 0 && (!qi || !qw || !cand || !ids || !scores))) { err = "rescore: n_queries >= 0 and query / candidate / result pointers required"; return -2; }
    return nq > 0;
}

}  // namespace

bool sparse_queries_ok(int nq, int kq, const int32_t *qids, const float *qw, int n_vocab, std::string &err) {
    return check_terms("search: query", nq, kq, qids, qw, n_vocab, false, err);
}

SparseIndex *SparseIndex::create(Engine *eng, int n_vocab, int width, int dtype, std::string &err) {
    if (!eng) { err = "no device engine"; return nullptr; }
    if (n_vocab < 1 || n_vocab > MAX_VOCAB) { err = "n_vocab must be 1 .. 262144"; return nullptr; }
    if (width < 1 || width > MAX_TERMS) { err = "width must be 1 .. 256"; return nullptr; }
    if (dtype < 0 || dtype > 1) { err = "dtype must be 0 (i32 ids, f32 weights) or 1 (u16 ids, f16 weights)"; return nullptr; }
    if (dtype == 1 && n_vocab > 65536) { err = "dtype 1 stores u16 ids: n_vocab must be at most 65536"; return nullptr; }
    DeviceGuard g(eng->device());
    SparseIndex *ix = new SparseIndex;
    ix->n_vocab_ = n_vocab;
    ix->width_ = width;
    ix->dtype_ = dtype;
    if (!ix->open(eng, "sparse index", err)) { delete ix; return nullptr; }
    sparse_index_kernels_init();
    return ix;
}

SparseIndex::~SparseIndex() {
    DeviceGuard g(eng_ ? eng_->device() : 0);
    close();
    if (sids_) (void)hipFree(sids_);
    if (sweights_) (void)hipFree(sweights_);
    if (counts_) (void)hipFree(counts_);
}

// (whole blocks: a block's layout does not depend on the capacity, so growth is three plain copies)
bool SparseIndex::grow_rows(int n_rows, std::string &err) {
    if (n_rows <= cap_) return true;
    const long long want = std::max<long long>({(long long)n_rows, (long long)cap_ * 3 / 2, 1024});
    const int cap = (int)std::min<long long>((long long)blocks_of(INT_MAX - SPARSE_BLOCK_ROWS) * SPARSE_BLOCK_ROWS, (long long)blocks_of(want) * SPARSE_BLOCK_ROWS);
    const size_t ib = sparse_id_bytes(dtype_), block_elems = (size_t)width_ * SPARSE_BLOCK_ROWS;
    const size_t nb = (size_t)cap / SPARSE_BLOCK_ROWS, used = (size_t)blocks_of(n_);
    void *pi = nullptr, *pw = nullptr;
    int32_t *pc = nullptr;
    HIP_OK(hipEventSynchronize(busy_), err, false);
    const char *failed = nullptr;
    // (an index with removed rows: the live words grow with the rows, so that an add within the capacity never allocates)
    uint32_t *lv = nullptr;
    if (hipMalloc(&pi, nb * block_elems * ib) != hipSuccess || hipMalloc(&pw, nb * block_elems * ib) != hipSuccess ||
        hipMalloc((void **)&pc, (size_t)cap * 4) != hipSuccess) failed = "hipMalloc (sparse index rows) failed";
    else if (n_ > 0 && (hipMemcpy(pi, sids_, used * block_elems * ib, hipMemcpyDeviceToDevice) != hipSuccess ||
                        hipMemcpy(pw, sweights_, used * block_elems * ib, hipMemcpyDeviceToDevice) != hipSuccess ||
                        hipMemcpy(pc, counts_, (size_t)n_ * 4, hipMemcpyDeviceToDevice) != hipSuccess)) failed = "hipMemcpy (sparse index rows) failed";
    if (failed) err = failed;
    if (failed || !live_for_capacity(cap, lv, err)) {
        (void)hipGetLastError();
        if (pi) (void)hipFree(pi);
        if (pw) (void)hipFree(pw);
        if (pc) (void)hipFree(pc);
        return false;
    }
    if (sids_) (void)hipFree(sids_);
    if (sweights_) (void)hipFree(sweights_);
    if (counts_) (void)hipFree(counts_);
    adopt_live(lv, cap);
    sids_ = pi; sweights_ = pw; counts_ = pc;
    cap_ = cap;
    return true;
}

bool SparseIndex::grow_search(int n_rows, int nqc, int k, std::string &err) {
    const size_t ent = ws_entries_bound(dtype_, n_vocab_, n_rows, nqc, k, eng_->options().sparse_index_qb);
    return grow(ws_s_, ent * 4, err) && grow(ws_i_, ent * 4, err) && grow(images_, (size_t)nqc * sparse_image_bytes(n_vocab_), err);
}

int SparseIndex::reserve(int n_rows, int n_queries, int k, std::string &err) {
    if (n_rows < 0 || n_queries < 0 || k < 1 || k > MAX_K) { err = "reserve: n_rows, n_queries >= 0 and 1 <= k <= 256 required"; return -2; }
    DeviceGuard g(eng_->device());
    if (!grow_rows(n_rows, err)) return -3;
    const int nqc = std::min(n_queries, QCHUNK);
    res_nq_ = nqc; res_k_ = k;
    if (nqc == 0) return 0;
    // (the entries grow with k — the list length, and so the tile, changes at k = 128, the slices only fall with it)
    size_t ent = 0;
    for (int kk : {std::min(k, 128), k}) ent = std::max(ent, ws_entries_bound(dtype_, n_vocab_, std::max(n_rows, n_), nqc, kk, eng_->options().sparse_index_qb));
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow(images_, (size_t)nqc * sparse_image_bytes(n_vocab_), err)) return -3;
    // (an index with postings: the inverted plan's workspace over the rows they cover)
    if (inverted_ && !grow_inverted(inv_rows_, nqc, k, err)) return -3;
    return 0;
}

int SparseIndex::add_device(int n, int k_in, const int32_t *d_ids, const float *d_weights, hipStream_t s, std::string &err) {
    if (const int go = check_add(n, k_in, d_ids, d_weights, width_, n_, err); go <= 0) return go < 0 ? go : n_;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;                                     // (engine.h: the one-event rule, and what a capturing stream changes)
    if (!eng_->op_begin(s, busy_, op, err)) return -3;
    if (!grow_rows(n_ + n, err)) return -3;
    SparseAddArgs a;
    a.ids = d_ids; a.weights = d_weights; a.sids = sids_; a.sweights = sweights_; a.counts = counts_;
    a.first = n_; a.n = n; a.k_in = k_in; a.width = width_; a.n_vocab = n_vocab_;
    eng_->timed_launch(dtype_ ? "sparse_index_add_f16" : "sparse_index_add_f32", 0.0, s, [&] { launch_sparse_add(dtype_, a, s); });
    // (rows added after a removal are live: their bits on the same stream, and in the mirror, which is already long enough)
    if (live_) launch_live_set_range(live_, n_, n, s);
    HIP_OK(hipGetLastError(), err, -3);
    if (!eng_->op_end(op, err)) return -3;
    if (live_) bits_.set_range(n_, n);
    const int first = n_;
    n_ += n;
    return first;
}

int SparseIndex::add_host(int n, int k_in, const int32_t *ids, const float *weights, std::string &err) {
    if (const int go = check_add(n, k_in, ids, weights, width_, n_, err); go <= 0) return go < 0 ? go : n_;
    if (!check_terms("add: row", n, k_in, ids, weights, n_vocab_, dtype_ == 1, err)) return -2;
    DeviceGuard g(eng_->device());
    const int first = n_;
    if (!grow_rows(n_ + n, err)) return -3;
    // through a staging buffer of at most 64 MiB (a row's stored form does not depend on the parts it came in)
    const size_t row_bytes = (size_t)k_in * 4;
    const int per = (int)std::max<size_t>(1, ((size_t)32 << 20) / row_bytes);
    for (int i0 = 0; i0 < n; i0 += per) {
        const int c = std::min(per, n - i0);
        const size_t half = ((size_t)c * row_bytes + 15) & ~(size_t)15;
        bool ok = grow(stage_, 2 * half, err);
        char *d = stage_.as<char>();
        ok = ok && hipStreamWaitEvent(stream_, busy_, 0) == hipSuccess &&
             hipMemcpyAsync(d, ids + (size_t)i0 * k_in, (size_t)c * row_bytes, hipMemcpyHostToDevice, stream_) == hipSuccess &&
             hipMemcpyAsync(d + half, weights + (size_t)i0 * k_in, (size_t)c * row_bytes, hipMemcpyHostToDevice, stream_) == hipSuccess &&
             add_device(c, k_in, (const int32_t *)d, (const float *)(d + half), stream_, err) >= 0 && hipStreamSynchronize(stream_) == hipSuccess;
        if (!ok) {
            (void)hipStreamSynchronize(stream_);
            if (err.empty()) err = "add: copy to the device failed";
            truncate(first);
            return -3;
        }
    }
    return first;
}

// the images of a chunk's queries into images_
void SparseIndex::enqueue_queries(int nq, int kq, const int32_t *d_qids, const float *d_qw, hipStream_t s) {
    SparseQueryArgs q;
    q.ids = d_qids; q.weights = d_qw; q.images = images_.as<char>(); q.nq = nq; q.kq = kq; q.n_vocab = n_vocab_;
    q.words = sparse_image_words(n_vocab_); q.img_bytes = (unsigned)sparse_image_bytes(n_vocab_);
    eng_->timed_launch("sparse_query", 0.0, s, [&] { launch_sparse_query(q, s); });
}

void SparseIndex::enqueue_chunk(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                                const uint32_t *d_allow) {
    SparseScanGeometry g;
    sparse_scan_geometry(dtype_, n_vocab_, n_, nq, k, g, eng_->options().sparse_index_qb);     // (create's bounds: never refused)
    const unsigned img = (unsigned)sparse_image_bytes(n_vocab_);
    enqueue_queries(nq, kq, d_qids, d_qw, s);
    const bool masked = live_ || d_allow;                    // (removed rows or an allow-list: the masked kernel, the same plan and workspace)
    SparseScanArgs a;
    a.sids = sids_; a.sweights = sweights_; a.counts = counts_; a.images = images_.as<char>();
    a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
    a.n_rows = n_; a.width = width_; a.nq = nq; a.qb = g.qb; a.n_qtiles = g.n_qtiles; a.n_slices = g.n_slices; a.slice_rows = g.slice_rows;
    a.k = k; a.L = g.L; a.n_items = g.n_qtiles * g.n_slices; a.words = sparse_image_words(n_vocab_); a.img_bytes = img;
    a.live = live_; a.allow = d_allow;
    static const char *const names[2][2] = {{"sparse_index_scan_f32", "sparse_index_scan_f32_masked"}, {"sparse_index_scan_f16", "sparse_index_scan_f16_masked"}};
    eng_->timed_launch(names[dtype_][masked], 0.0, s, [&] { launch_sparse_scan(dtype_, a, g.lds, s); });
    enqueue_merge(nq, g.n_slices * k, k, d_ids, d_scores, s);
}

int SparseIndex::search_device(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                               std::string &err, const uint32_t *d_allow, bool inverted) {
    if (const int go = check_search(nq, kq, d_qids, d_qw, k, d_ids, d_scores, err); go <= 0) return go;
    if (inverted && !inverted_ok(err)) return -2;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -3;
    if (!(inverted ? grow_inverted(n_, std::min(nq, QCHUNK), k, err) : grow_search(n_, std::min(nq, QCHUNK), k, err))) return -3;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        if (inverted) enqueue_chunk_inverted(c, kq, d_qids + (size_t)c0 * kq, d_qw + (size_t)c0 * kq, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s, d_allow);
        else enqueue_chunk(c, kq, d_qids + (size_t)c0 * kq, d_qw + (size_t)c0 * kq, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s, d_allow);
    }
    HIP_OK(hipGetLastError(), err, -3);
    return eng_->op_end(op, err) ? 0 : -3;
}

int SparseIndex::search_device_to_host(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *ids, float *scores, std::string &err,
                                       const uint32_t *d_allow, bool inverted) {
    if (inverted && !inverted_ok(err)) return -2;
    HostResults res((size_t)nq * k);
    if (!grow(out_ids_, res.ids.size() * 4, err) || !grow(out_scores_, res.scores.size() * 4, err)) return -3;
    if (search_device(nq, kq, d_qids, d_qw, k, out_ids_.as<int32_t>(), out_scores_.as<float>(), stream_, err, d_allow, inverted) != 0) { (void)hipStreamSynchronize(stream_); return -3; }
    if (!results_to_host(stream_, 0, res.ids.size(), res, err)) return -3;
    res.deliver(ids, scores);
    return 0;
}

int SparseIndex::search_host(int nq, int kq, const int32_t *qids, const float *qw, int k, int32_t *ids, float *scores, std::string &err,
                             const uint32_t *allow, bool inverted) {
    if (const int go = check_search(nq, kq, qids, qw, k, ids, scores, err); go <= 0) return go;
    if (!check_terms("search: query", nq, kq, qids, qw, n_vocab_, false, err)) return -2;
    if (inverted && !inverted_ok(err)) return -2;
    DeviceGuard g(eng_->device());
    const uint32_t *d_allow = nullptr;
    if (!upload_allow(allow, stream_, d_allow, err)) return -3;
    HostResults res((size_t)nq * k);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const size_t half = ((size_t)c * kq * 4 + 15) & ~(size_t)15;
        if (!grow(stage_, 2 * half, err)) return -3;
        char *d = stage_.as<char>();
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -3);
        HIP_OK(hipMemcpyAsync(d, qids + (size_t)c0 * kq, (size_t)c * kq * 4, hipMemcpyHostToDevice, stream_), err, -3);
        HIP_OK(hipMemcpyAsync(d + half, qw + (size_t)c0 * kq, (size_t)c * kq * 4, hipMemcpyHostToDevice, stream_), err, -3);
        if (search_device_to_host(c, kq, (const int32_t *)d, (const float *)(d + half), k, res.ids.data() + (size_t)c0 * k, res.scores.data() + (size_t)c0 * k, err, d_allow, inverted) != 0) return -3;
    }
    res.deliver(ids, scores);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// rescoring
// ------------------------------------------------------------------------------------------------
int SparseIndex::rescore_device(int nq, int kq, const int32_t *d_qids, const float *d_qw, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids,
                                float *d_scores, hipStream_t s, std::string &err) {
    if (const int go = check_rescore(nq, kq, d_qids, d_qw, n_cand, d_cand, k, d_ids, d_scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -3;
    const int nqc = std::min(nq, QCHUNK);
    const size_t ent = (size_t)nqc * n_cand;
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow(images_, (size_t)nqc * sparse_image_bytes(n_vocab_), err)) return -3;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        enqueue_queries(c, kq, d_qids + (size_t)c0 * kq, d_qw + (size_t)c0 * kq, s);
        SparseRescoreArgs a;
        a.sids = sids_; a.sweights = sweights_; a.counts = counts_; a.images = images_.as<char>(); a.live = live_;
        a.cand = d_cand + (size_t)c0 * n_cand; a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
        a.n_rows = n_; a.width = width_; a.nq = c; a.n_cand = n_cand; a.n_chunks = (n_cand + SPARSE_RESCORE_CAND - 1) / SPARSE_RESCORE_CAND;
        a.words = sparse_image_words(n_vocab_); a.img_bytes = (unsigned)sparse_image_bytes(n_vocab_);
        eng_->timed_launch(dtype_ ? "sparse_index_rescore_f16" : "sparse_index_rescore_f32", 0.0, s, [&] { launch_sparse_rescore(dtype_, a, s); });
        enqueue_merge(c, n_cand, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
    }
    HIP_OK(hipGetLastError(), err, -3);
    return eng_->op_end(op, err) ? 0 : -3;
}

int SparseIndex::rescore_to_host(int nq, int kq, const int32_t *qids, const float *qw, int n_cand, const int32_t *cand, int k, int32_t *ids,
                                 float *scores, std::string &err) {
    if (const int go = check_rescore(nq, kq, qids, qw, n_cand, cand, k, ids, scores, err); go <= 0) return go;
    if (!check_terms("rescore: query", nq, kq, qids, qw, n_vocab_, false, err)) return -2;
    for (size_t i = 0; i < (size_t)nq * n_cand; ++i)
        if (cand[i] < -1 || cand[i] >= n_) { err = "rescore: candidate id " + std::to_string(cand[i]) + " is outside [-1, " + std::to_string(n_) + ")"; return -2; }
    DeviceGuard g(eng_->device());
    HostResults res((size_t)nq * k);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const size_t half = ((size_t)c * kq * 4 + 15) & ~(size_t)15;
        if (!grow(stage_, 2 * half, err) || !grow(cand_in_, (size_t)c * n_cand * 4, err) || !grow(out_ids_, (size_t)c * k * 4, err) ||
            !grow(out_scores_, (size_t)c * k * 4, err)) return -3;
        char *d = stage_.as<char>();
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -3);
        HIP_OK(hipMemcpyAsync(d, qids + (size_t)c0 * kq, (size_t)c * kq * 4, hipMemcpyHostToDevice, stream_), err, -3);
        HIP_OK(hipMemcpyAsync(d + half, qw + (size_t)c0 * kq, (size_t)c * kq * 4, hipMemcpyHostToDevice, stream_), err, -3);
        HIP_OK(hipMemcpyAsync(cand_in_.p, cand + (size_t)c0 * n_cand, (size_t)c * n_cand * 4, hipMemcpyHostToDevice, stream_), err, -3);
        if (rescore_device(c, kq, (const int32_t *)d, (const float *)(d + half), n_cand, cand_in_.as<int32_t>(), k, out_ids_.as<int32_t>(),
                           out_scores_.as<float>(), stream_, err) != 0) { (void)hipStreamSynchronize(stream_); return -3; }
        if (!results_to_host(stream_, (size_t)c0 * k, (size_t)c * k, res, err)) return -3;
    }
    res.deliver(ids, scores);
    return 0;
}

int SparseIndex::get_rows(int n, const int32_t *row_ids, int32_t *out_ids, float *out_weights, std::string &err) {
    if (n < 0 || (n > 0 && (!row_ids || !out_ids || !out_weights))) { err = "get_rows: n >= 0 and row id / output pointers required"; return -2; }
    for (int i = 0; i < n; ++i)
        if (row_ids[i] < 0 || row_ids[i] >= n_) { err = "get_rows: row id " + std::to_string(row_ids[i]) + " outside [0, " + std::to_string(n_) + ")"; return -2; }
    if (n == 0) return 0;
    DeviceGuard g(eng_->device());
    // in parts whose results fit 32 MiB
    const int per = (int)std::max<size_t>(1, ((size_t)32 << 20) / ((size_t)width_ * 8));
    std::vector<int32_t> hid((size_t)std::min(per, n) * width_);
    std::vector<float> hw(hid.size());
    for (int i0 = 0; i0 < n; i0 += per) {
        const int c = std::min(per, n - i0);
        const size_t m = (size_t)c * width_;
        if (!grow(stage_, (size_t)c * 4, err) || !grow(out_ids_, m * 4, err) || !grow(out_scores_, m * 4, err)) return -3;
        Engine::StreamOp op;
        if (!eng_->op_begin(stream_, busy_, op, err)) return -3;
        HIP_OK(hipMemcpyAsync(stage_.p, row_ids + i0, (size_t)c * 4, hipMemcpyHostToDevice, stream_), err, -3);
        SparseExportArgs a;
        a.sids = sids_; a.sweights = sweights_; a.counts = counts_; a.rows = stage_.as<int32_t>();
        a.out_ids = out_ids_.as<int32_t>(); a.out_weights = out_scores_.as<float>(); a.n = c; a.width = width_;
        eng_->timed_launch(dtype_ ? "sparse_index_export_f16" : "sparse_index_export_f32", 0.0, stream_, [&] { launch_sparse_export(dtype_, a, stream_); });
        HIP_OK(hipGetLastError(), err, -3);
        HIP_OK(hipMemcpyAsync(hid.data(), out_ids_.p, m * 4, hipMemcpyDeviceToHost, stream_), err, -3);
        HIP_OK(hipMemcpyAsync(hw.data(), out_scores_.p, m * 4, hipMemcpyDeviceToHost, stream_), err, -3);
        if (!eng_->op_end(op, err)) return -3;
        HIP_OK(hipStreamSynchronize(stream_), err, -3);
        memcpy(out_ids + (size_t)i0 * width_, hid.data(), m * 4);
        memcpy(out_weights + (size_t)i0 * width_, hw.data(), m * 4);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// removed rows, compaction, file form
// ------------------------------------------------------------------------------------------------
void SparseIndex::truncate(int n) {
    if (n < 0 || n >= n_) return;
    if (inverted_ && n < inv_rows_) drop_postings();
    if (live_) bits_.truncate(n_, n);                        // (live_bits.h: the mirror's side of the invariant; the device words stay)
    n_ = n;
}

int SparseIndex::remove(int n, const int32_t *ids, std::string &err) {
    std::vector<int32_t> fresh;                          // the ids this call removes (repeats and removed rows left out)
    const Removed r = remove_rows(n, ids, cap_, fresh, err);
    return r == Removed::ok ? (int)fresh.size() : r == Removed::refused ? -2 : -3;
}

int SparseIndex::compact(int32_t *old_ids, std::string &err) {
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -3);
    drop_postings();                                         // (the ids change: invert again)
    if (bits_.n_removed == 0) return compact_nothing(old_ids);
    const std::vector<int32_t> map = bits_.kept(n_);
    const int nl = (int)map.size();
    const size_t arr = (size_t)blocks_of(nl) * width_ * SPARSE_BLOCK_ROWS * sparse_id_bytes(dtype_);
    const int cap = blocks_of(nl) * SPARSE_BLOCK_ROWS;
    void *pi = nullptr, *pw = nullptr;
    int32_t *pc = nullptr, *d_map = nullptr;
    const char *failed = nullptr;
    if (nl > 0) {
        if (hipMalloc(&pi, arr) != hipSuccess || hipMalloc(&pw, arr) != hipSuccess || hipMalloc((void **)&pc, (size_t)cap * 4) != hipSuccess ||
            hipMalloc((void **)&d_map, (size_t)nl * 4) != hipSuccess) failed = "hipMalloc (sparse index rows) failed";
        else if (hipMemcpyAsync(d_map, map.data(), (size_t)nl * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) failed = "hipMemcpy (compaction ids) failed";
        else {
            SparseGatherArgs a;
            a.sids = sids_; a.sweights = sweights_; a.counts = counts_; a.old_ids = d_map; a.dids = pi; a.dweights = pw; a.dcounts = pc;
            a.n = nl; a.width = width_;
            eng_->timed_launch(dtype_ ? "sparse_index_gather_f16" : "sparse_index_gather_f32", 0.0, stream_, [&] { launch_sparse_gather(dtype_, a, stream_); });
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) failed = "the gather kernel failed";
        }
        if (d_map) (void)hipFree(d_map);
        if (failed) {
            (void)hipGetLastError();
            if (pi) (void)hipFree(pi);
            if (pw) (void)hipFree(pw);
            if (pc) (void)hipFree(pc);
            err = failed;
            return -3;
        }
    }
    if (sids_) (void)hipFree(sids_);
    if (sweights_) (void)hipFree(sweights_);
    if (counts_) (void)hipFree(counts_);
    sids_ = pi; sweights_ = pw; counts_ = pc;
    cap_ = nl > 0 ? cap : 0;
    n_ = nl;
    drop_live();
    if (old_ids) memcpy(old_ids, map.data(), (size_t)nl * 4);
    return nl;
}

namespace {

// device memory <-> file in pieces of at most 64 MiB through a host buffer (index_io.h)
constexpr size_t FILE_PIECE = (size_t)64 << 20;

// one of the two block arrays of n rows: the whole blocks as they are, the last, partial one with its rows at and beyond n zeroed
bool blocks_to_file(FILE *f, const void *d, int n, int width, size_t eb, std::vector<char> &buf, std::string &err) {
    const size_t block = (size_t)width * SPARSE_BLOCK_ROWS * eb, whole = (size_t)(n / SPARSE_BLOCK_ROWS);
    if (!device_to_file(f, d, whole * block, FILE_PIECE, buf, err)) return false;
    const int rest = n % SPARSE_BLOCK_ROWS;
    if (rest == 0) return true;
    std::vector<char> last(block);
    HIP_OK(hipMemcpy(last.data(), (const char *)d + whole * block, block, hipMemcpyDeviceToHost), err, false);
    for (int j = 0; j < width; ++j) memset(last.data() + ((size_t)j * SPARSE_BLOCK_ROWS + rest) * eb, 0, (size_t)(SPARSE_BLOCK_ROWS - rest) * eb);
    if (fwrite(last.data(), 1, block, f) != block) { err = "write failed"; return false; }
    return true;
}

}  // namespace

bool SparseIndex::save(const char *path, std::string &err) {
    if (!path || !*path) { err = "a path is required"; return false; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, false);
    SparseIndexFileHeader h;
    h.dtype = (uint32_t)dtype_; h.n_vocab = (uint32_t)n_vocab_; h.width = (uint32_t)width_; h.n_rows = (uint32_t)n_; h.has_live = live_ ? 1u : 0u;
    unsigned char hdr[INDEX_HEADER_BYTES];
    sparse_index_header_write(h, hdr);
    return write_atomically(path, err, [&](FILE *f) {
        std::vector<char> buf;
        const size_t eb = sparse_id_bytes(dtype_);
        // (the live words come from the mirror: its bits at and beyond size are zero)
        return fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr && blocks_to_file(f, sids_, n_, width_, eb, buf, err) &&
               blocks_to_file(f, sweights_, n_, width_, eb, buf, err) && device_to_file(f, counts_, (size_t)n_ * 4, FILE_PIECE, buf, err) &&
               (!live_ || fwrite(bits_.words.data(), 4, live_words(n_), f) == live_words(n_));
    });
}

SparseIndex *SparseIndex::load(Engine *eng, FILE *f, const SparseIndexFileHeader &h, std::string &err) {
    const int n = (int)h.n_rows;
    const uint64_t arr = sparse_index_file_array_bytes(h);
    // the counts stand behind the two arrays: read and checked first, since the id check needs them
    std::vector<int32_t> counts((size_t)n);
    if (fseeko(f, (off_t)(INDEX_HEADER_BYTES + 2 * arr), SEEK_SET) != 0 || fread(counts.data(), 4, counts.size(), f) != counts.size()) { err = "read failed"; return nullptr; }
    if (!sparse_index_counts_check(h, counts.data(), err)) return nullptr;
    std::vector<uint32_t> words(h.has_live ? live_words(n) : 0);
    if (fread(words.data(), 4, words.size(), f) != words.size()) { err = "read failed"; return nullptr; }
    if (!sparse_index_live_check(h, words.data(), err)) return nullptr;
    // the ids, in pieces of whole blocks, each checked against the counts in front of any allocation
    const size_t block = (size_t)h.width * SPARSE_BLOCK_ROWS * sparse_id_bytes((int)h.dtype);
    const size_t per = std::max<size_t>(1, FILE_PIECE / block), nb = (size_t)blocks_of(n);
    std::vector<char> buf(std::min(per, std::max<size_t>(nb, 1)) * block);
    if (fseeko(f, (off_t)INDEX_HEADER_BYTES, SEEK_SET) != 0) { err = "read failed"; return nullptr; }
    for (size_t b0 = 0; b0 < nb; b0 += per) {
        const size_t c = std::min(per, nb - b0);
        if (fread(buf.data(), 1, c * block, f) != c * block) { err = "read failed"; return nullptr; }
        if (!sparse_index_ids_check(h, buf.data(), b0, c, counts.data(), err)) return nullptr;
    }
    std::unique_ptr<SparseIndex> ix(create(eng, (int)h.n_vocab, (int)h.width, (int)h.dtype, err));
    if (!ix) return nullptr;
    DeviceGuard g(eng->device());
    if (n == 0) return ix.release();
    if (!ix->grow_rows(n, err)) return nullptr;
    if (fseeko(f, (off_t)INDEX_HEADER_BYTES, SEEK_SET) != 0) { err = "read failed"; return nullptr; }
    for (void *dst : {ix->sids_, ix->sweights_})
        if (!file_to_device(f, dst, nb * block, per * block, buf, err)) return nullptr;
    HIP_OK(hipMemcpy(ix->counts_, counts.data(), (size_t)n * 4, hipMemcpyHostToDevice), err, nullptr);
    ix->n_ = n;
    if (!h.has_live) return ix.release();
    if (!ix->install_live(words.data(), ix->cap_, err)) return nullptr;
    return ix.release();
}

bool SparseIndex::text_buffers(size_t in_bytes, size_t out_bytes, char *&d_in, char *&d_out, std::string &err) {
    if (!grow(text_in_, in_bytes, err) || !grow(text_out_, out_bytes, err)) return false;
    d_in = text_in_.as<char>();
    d_out = text_out_.as<char>();
    return true;
}

}  // namespace bert_hip
