// sparse_postings.cpp — the sparse index's postings and inverted search, host side (sparse_index.h): building the term-major image
// from the stored blocks, its life cycle, the workspace of the inverted plan and the launches of one chunk of queries.  The kernels
// are in sparse_postings.hip (and the merge in search.hip), reached through sparse_index_kernels.h / search_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "sparse_index.h"

namespace bert_hip {

namespace {

// the sorted queries of a chunk: ids [nqc][256] i32 | weights [nqc][256] f32 | counts [nqc] i32
size_t qterms_bytes(int nqc) { return (size_t)nqc * (SPARSE_MAX_TERMS * 8 + 4); }

// the most workspace entries (nq' * slices * k) a chunk of up to nqc queries takes under the inverted plan
size_t inverted_entries_bound(int dtype, int n_vocab, int n_rows, int nqc, int k, int seg, int qb_pref) {
    size_t ent = 0;
    SparsePostingsGeometry g;
    for (int q = 1; q <= nqc; ++q)
        if (sparse_postings_geometry(dtype, n_vocab, n_rows, q, k, seg, g, qb_pref)) ent = std::max(ent, (size_t)q * g.max_slices * k);
    return ent;
}

}  // namespace

void SparseIndex::drop_postings() {
    // (the buffers stay: grow-only, like the workspace)
    inverted_ = false;
    inv_rows_ = 0;
}

bool SparseIndex::inverted_ok(std::string &err) const {
    if (!inverted_) { err = "search_inverted: the index has no postings: call bert_hip_sparse_index_invert first"; return false; }
    if (inv_rows_ != n_) {
        err = "search_inverted: the postings cover " + std::to_string(inv_rows_) + " of " + std::to_string(n_) +
              " rows (rows were added since): call bert_hip_sparse_index_invert again";
        return false;
    }
    return true;
}

bool SparseIndex::grow_inverted(int n_rows, int nqc, int k, std::string &err) {
    if (nqc < 1) return true;
    // (as reserve: the list length, and with it the tile, changes at k = 128)
    size_t ent = 0;
    for (int kk : {std::min(k, 128), k})
        ent = std::max(ent, inverted_entries_bound(dtype_, n_vocab_, n_rows, nqc, kk, inv_seg_, eng_->options().sparse_index_qb));
    return grow(ws_s_, ent * 4, err) && grow(ws_i_, ent * 4, err) && grow(qterms_, qterms_bytes(nqc), err);
}

int SparseIndex::invert(std::string &err) {
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -3);
    sparse_postings_kernels_init();
    const int seg = sparse_segment_rows(eng_->options().sparse_index_segment_rows);
    const int n_segs = sparse_segments(n_, seg);
    drop_postings();
    inv_seg_ = seg;
    if (n_ > 0) {
        const size_t off_bytes = (size_t)n_segs * (n_vocab_ + 1) * 4, slots = (size_t)n_segs * seg * width_;
        DevBuf cur;                                          // the fill's cursors: a copy of the offsets, gone afterwards
        if (!poff_.ensure(off_bytes, err) || !prow_.ensure(slots * 2, err) || !pw_.ensure(slots * (dtype_ == 1 ? 2 : 4), err) ||
            !cur.ensure(off_bytes, err)) return -3;
        SparsePostingsBuildArgs a;
        a.sids = sids_; a.sweights = sweights_; a.counts = counts_; a.off = poff_.as<uint32_t>(); a.cur = cur.as<uint32_t>();
        a.prow = prow_.as<uint16_t>(); a.pw = pw_.p; a.n_rows = n_; a.width = width_; a.n_vocab = n_vocab_; a.seg = seg;
        launch_sparse_postings_build(dtype_, a, stream_);
        HIP_OK(hipGetLastError(), err, -3);
        HIP_OK(hipStreamSynchronize(stream_), err, -3);
    }
    inverted_ = true;
    inv_rows_ = n_;
    if (!grow_inverted(n_, res_nq_, res_k_, err)) { drop_postings(); return -3; }
    return n_;
}

void SparseIndex::enqueue_chunk_inverted(int nq, int kq, const int32_t *d_qids, const float *d_qw, int k, int32_t *d_ids, float *d_scores,
                                         hipStream_t s, const uint32_t *d_allow) {
    SparsePostingsGeometry g;
    sparse_postings_geometry(dtype_, n_vocab_, n_, nq, k, inv_seg_, g, eng_->options().sparse_index_qb);   // (create's and invert's bounds: never refused)
    // the chunk's queries, sorted: the three parts of qterms_ at the chunk's own size
    int32_t *tids = qterms_.as<int32_t>();
    float *tw = (float *)(tids + (size_t)nq * SPARSE_MAX_TERMS);
    int32_t *tn = (int32_t *)(tw + (size_t)nq * SPARSE_MAX_TERMS);
    SparseQuerySortArgs q;
    q.ids = d_qids; q.weights = d_qw; q.tids = tids; q.tw = tw; q.tn = tn; q.nq = nq; q.kq = kq; q.n_vocab = n_vocab_;
    eng_->timed_launch("sparse_query_sort", 0.0, s, [&] { launch_sparse_query_sort(q, s); });
    const bool masked = live_ || d_allow;
    SparsePostingsScanArgs a;
    a.off = poff_.as<uint32_t>(); a.prow = prow_.as<uint16_t>(); a.pw = pw_.p; a.tids = tids; a.tw = tw; a.tn = tn;
    a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
    a.n_rows = n_; a.width = width_; a.n_vocab = n_vocab_; a.seg = inv_seg_; a.nq = nq; a.qb = g.qb; a.n_qtiles = g.n_qtiles;
    a.n_slices = g.n_slices; a.slice_segs = g.slice_segs; a.k = k; a.L = g.L; a.n_items = g.n_qtiles * g.n_slices;
    a.live = live_; a.allow = d_allow;
    static const char *const names[2][2] = {{"sparse_postings_scan_f32", "sparse_postings_scan_f32_masked"}, {"sparse_postings_scan_f16", "sparse_postings_scan_f16_masked"}};
    eng_->timed_launch(names[dtype_][masked], 0.0, s, [&] { launch_sparse_postings_scan(dtype_, a, g.lds, s); });
    enqueue_merge(nq, g.n_slices * k, k, d_ids, d_scores, s);
}

int SparseIndex::postings_segment_host(int sg, std::vector<uint32_t> &off, std::vector<uint16_t> &rows, std::vector<float> &weights, std::string &err) {
    if (!inverted_ || sg < 0 || sg >= sparse_segments(inv_rows_, inv_seg_)) { err = "no postings, or no such segment"; return -2; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -3);
    off.resize((size_t)n_vocab_ + 1);
    HIP_OK(hipMemcpy(off.data(), poff_.as<uint32_t>() + (size_t)sg * (n_vocab_ + 1), off.size() * 4, hipMemcpyDeviceToHost), err, -3);
    const size_t per_seg = (size_t)inv_seg_ * width_, total = std::min<size_t>(off.back(), per_seg);
    rows.resize(total);
    weights.resize(total);
    if (total == 0) return 0;
    HIP_OK(hipMemcpy(rows.data(), prow_.as<uint16_t>() + (size_t)sg * per_seg, total * 2, hipMemcpyDeviceToHost), err, -3);
    if (dtype_ == 1) {
        std::vector<half_t> h(total);
        HIP_OK(hipMemcpy(h.data(), pw_.as<half_t>() + (size_t)sg * per_seg, total * 2, hipMemcpyDeviceToHost), err, -3);
        for (size_t i = 0; i < total; ++i) weights[i] = (float)h[i];
    } else {
        HIP_OK(hipMemcpy(weights.data(), pw_.as<float>() + (size_t)sg * per_seg, total * 4, hipMemcpyDeviceToHost), err, -3);
    }
    return (int)total;
}

}  // namespace bert_hip
