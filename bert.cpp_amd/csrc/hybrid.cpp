// hybrid.cpp — the host side of hybrid search (hybrid.h): the checks, the workspace, the chunks of a device call and their launches,
// the host route and the route of the text entry.  The kernels are index_scores_kernel and mask_and_kernel (search.hip), then one of
// two scan arms — over the rows sparse_query_kernel and sparse_hybrid_scan_kernel (sparse_index.hip), over the postings
// sparse_query_sort_kernel and sparse_postings_hybrid_scan_kernel (sparse_postings.hip) — and topk_merge_kernel (search.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "hybrid.h"
#include "search_kernels.h"
#include "sparse_index_kernels.h"

namespace bert_hip {

namespace {

// the profiler's names, by the dense index's dtype / the sparse index's dtype, plain and masked
const char *const SCORES_NAMES[4][2] = {{"index_scores_f32", "index_scores_f32_masked"}, {"index_scores_f16", "index_scores_f16_masked"},
                                        {"index_scores_i8", "index_scores_i8_masked"}, {"index_scores_b1", "index_scores_b1_masked"}};
const char *const SCAN_NAMES[2][2] = {{"sparse_hybrid_scan_f32", "sparse_hybrid_scan_f32_masked"}, {"sparse_hybrid_scan_f16", "sparse_hybrid_scan_f16_masked"}};
const char *const POSTINGS_SCAN_NAMES[2][2] = {{"sparse_postings_hybrid_scan_f32", "sparse_postings_hybrid_scan_f32_masked"},
                                               {"sparse_postings_hybrid_scan_f16", "sparse_postings_hybrid_scan_f16_masked"}};

}  // namespace

int Hybrid::check(const Index &d, const SparseIndex &sp, int nq, bool have_ptrs, int kq, float w_dense, float w_sparse, const void *allow,
                  int n_words, int k, std::string &err, bool inverted) {
    if (d.eng_->device() != sp.eng_->device()) { err = "the two indexes live on different devices"; return -2; }
    if (d.size() != sp.size()) { err = "the embedding index holds " + std::to_string(d.size()) + " rows, the sparse index " + std::to_string(sp.size()); return -2; }
    if (k < 1 || k > SparseIndex::MAX_K) { err = "k must be 1 .. 256"; return -2; }
    if (kq < 1 || kq > SparseIndex::MAX_TERMS) { err = "kq must be 1 .. 256"; return -2; }
    if (!std::isfinite(w_dense) || !std::isfinite(w_sparse)) { err = "w_dense and w_sparse must be finite"; return -2; }
    if (allow && (long long)n_words < (long long)live_words(sp.size())) {
        err = "the allow-list has " + std::to_string(n_words) + " words, indexes of " + std::to_string(sp.size()) + " rows need " + std::to_string(live_words(sp.size()));
        return -2;
    }
    if (nq < 0 || (nq > 0 && !have_ptrs)) { err = "n_queries >= 0 and query / result pointers required"; return -2; }
    // (as the inverted search: postings that cover every row, or nothing is answered)
    if (nq > 0 && inverted && !sp.inverted_ok(err)) return -2;
    return nq > 0;
}

int Hybrid::reserve(Index &d, SparseIndex &sp, int n_rows, int n_queries, int k, std::string &err) {
    if (d.eng_->device() != sp.eng_->device()) { err = "the two indexes live on different devices"; return -2; }
    if (n_rows < 0 || n_queries < 0 || k < 1 || k > SparseIndex::MAX_K) { err = "reserve: n_rows, n_queries >= 0 and 1 <= k <= 256 required"; return -2; }
    if (!d.reserve(n_rows, n_queries, k, err)) return -3;
    if (const int r = sp.reserve(n_rows, n_queries, k, err); r != 0) return r;
    DeviceGuard g(sp.eng_->device());
    const int rows = std::max({n_rows, d.size(), sp.size()});
    const size_t ld = hybrid_ld(rows);
    // a chunk's matrix is at most HYBRID_SCORES_MAX, or one query's scores where those alone exceed it; never more than every query's
    const size_t bytes = std::min((size_t)std::min(n_queries, Index::QCHUNK) * ld * 4, std::max(HYBRID_SCORES_MAX, ld * 4));
    if (!sp.grow(sp.hyb_scores_, bytes, err) || !sp.grow(sp.hyb_mask_, live_words(rows) * 4, err)) return -3;
    return 0;
}

int Hybrid::search_device(Index &d, SparseIndex &sp, int nq, const float *d_q, int kq, const int32_t *d_qids, const float *d_qw, float w_dense,
                          float w_sparse, const uint32_t *d_allow, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                          bool inverted) {
    if (nq <= 0) return 0;
    DeviceGuard g(sp.eng_->device());
    // one operation of both indexes (engine.h: the one-event rule, and what a capturing stream changes)
    Engine::StreamOp od, os;
    if (!d.eng_->op_begin(s, d.busy_, od, err) || !sp.eng_->op_begin(s, sp.busy_, os, err)) return -3;
    const int n = sp.n_;
    const int hc = hybrid_chunk_queries(n, nq, sp.eng_->options().hybrid_chunk_queries);
    const size_t ld = hybrid_ld(n), words = live_words(n);
    const bool masked = n > 0 && (d.live_ || sp.live_ || d_allow);
    if (!(inverted ? sp.grow_inverted(n, hc, k, err) : sp.grow_search(n, hc, k, err)) || !d.grow_queries(hc, err) || !sp.grow(sp.hyb_scores_, (size_t)hc * ld * 4, err) ||
        (masked && !sp.grow(sp.hyb_mask_, words * 4, err))) return -3;
    // the rows that qualify: live in both and allowed — one bitmap, the only mask of both passes
    const uint32_t *mask = nullptr;
    if (masked) {
        uint32_t *m = sp.hyb_mask_.as<uint32_t>();
        sp.eng_->timed_launch("mask_and", 0.0, s, [&] { launch_mask_and(d.live_, sp.live_, d_allow, m, (int)words, s); });
        mask = m;
    }
    SparseScanGeometry geo;
    const unsigned img = (unsigned)sparse_image_bytes(sp.n_vocab_);
    for (int c0 = 0; c0 < nq; c0 += hc) {
        const int c = std::min(hc, nq - c0);
        // the dense pass (an empty pair has no scores: the scan below reads none)
        if (n > 0) {
            d.enqueue_queries(c, d_q + (size_t)c0 * d.dim_, s);
            ScoresArgs a;
            a.rows = d.rows_; a.queries = d.qbuf_.p; a.qscale = d.qscale_.as<float>(); a.rscale = d.rscale_; a.mask = mask;
            a.out = sp.hyb_scores_.as<float>(); a.ld = ld; a.dpad = d.dpad_;
            index_scores_plan(n, c, a);
            d.eng_->timed_launch(SCORES_NAMES[d.dtype_][masked], 2.0 * c * (double)n * d.dim_, s, [&] { launch_index_scores(d.dtype_, a, s); });
        }
        if (inverted) {
            // the sparse pass over the postings: the chunk's sorted queries, the inverted plan, the selection by H
            SparsePostingsGeometry pg;
            sparse_postings_geometry(sp.dtype_, sp.n_vocab_, n, c, k, sp.inv_seg_, pg, sp.eng_->options().sparse_index_qb);   // (create's and invert's bounds: never refused)
            int32_t *tids = sp.qterms_.as<int32_t>();
            float *tw = (float *)(tids + (size_t)c * SPARSE_MAX_TERMS);
            int32_t *tn = (int32_t *)(tw + (size_t)c * SPARSE_MAX_TERMS);
            SparseQuerySortArgs q;
            q.ids = d_qids + (size_t)c0 * kq; q.weights = d_qw + (size_t)c0 * kq; q.tids = tids; q.tw = tw; q.tn = tn;
            q.nq = c; q.kq = kq; q.n_vocab = sp.n_vocab_;
            sp.eng_->timed_launch("sparse_query_sort", 0.0, s, [&] { launch_sparse_query_sort(q, s); });
            SparsePostingsScanArgs a;
            a.off = sp.poff_.as<uint32_t>(); a.prow = sp.prow_.as<uint16_t>(); a.pw = sp.pw_.p; a.tids = tids; a.tw = tw; a.tn = tn;
            a.ws_s = sp.ws_s_.as<float>(); a.ws_i = sp.ws_i_.as<int>();
            a.n_rows = n; a.width = sp.width_; a.n_vocab = sp.n_vocab_; a.seg = sp.inv_seg_; a.nq = c; a.qb = pg.qb; a.n_qtiles = pg.n_qtiles;
            a.n_slices = pg.n_slices; a.slice_segs = pg.slice_segs; a.k = k; a.L = pg.L; a.n_items = pg.n_qtiles * pg.n_slices;
            a.live = mask; a.allow = nullptr;
            a.dscores = sp.hyb_scores_.as<float>(); a.ld = ld; a.w_dense = w_dense; a.w_sparse = w_sparse;
            sp.eng_->timed_launch(POSTINGS_SCAN_NAMES[sp.dtype_][masked], 0.0, s, [&] { launch_sparse_postings_hybrid_scan(sp.dtype_, a, pg.lds, s); });
            sp.enqueue_merge(c, pg.n_slices * k, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
            continue;
        }
        // the sparse pass over the rows: the scan's plan, lists and images, the selection by H
        sparse_scan_geometry(sp.dtype_, sp.n_vocab_, n, c, k, geo, sp.eng_->options().sparse_index_qb);      // (create's bounds: never refused)
        sp.enqueue_queries(c, kq, d_qids + (size_t)c0 * kq, d_qw + (size_t)c0 * kq, s);
        SparseScanArgs a;
        a.sids = sp.sids_; a.sweights = sp.sweights_; a.counts = sp.counts_; a.images = sp.images_.as<char>();
        a.ws_s = sp.ws_s_.as<float>(); a.ws_i = sp.ws_i_.as<int>();
        a.n_rows = n; a.width = sp.width_; a.nq = c; a.qb = geo.qb; a.n_qtiles = geo.n_qtiles; a.n_slices = geo.n_slices; a.slice_rows = geo.slice_rows;
        a.k = k; a.L = geo.L; a.n_items = geo.n_qtiles * geo.n_slices; a.words = sparse_image_words(sp.n_vocab_); a.img_bytes = img;
        a.live = mask; a.allow = nullptr;
        a.dscores = sp.hyb_scores_.as<float>(); a.ld = ld; a.w_dense = w_dense; a.w_sparse = w_sparse;
        sp.eng_->timed_launch(SCAN_NAMES[sp.dtype_][masked], 0.0, s, [&] { launch_sparse_hybrid_scan(sp.dtype_, a, geo.lds, s); });
        sp.enqueue_merge(c, geo.n_slices * k, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
    }
    HIP_OK(hipGetLastError(), err, -3);
    return d.eng_->op_end(od, err) && sp.eng_->op_end(os, err) ? 0 : -3;
}

int Hybrid::search_device_to_host(Index &d, SparseIndex &sp, int nq, const float *d_q, int kq, const int32_t *d_qids, const float *d_qw,
                                  float w_dense, float w_sparse, int k, int32_t *ids, float *scores, std::string &err, bool inverted) {
    if (nq <= 0) return 0;
    DeviceGuard g(sp.eng_->device());
    hipStream_t s = sp.stream_;
    HostResults res((size_t)nq * k);
    if (!sp.grow(sp.out_ids_, res.ids.size() * 4, err) || !sp.grow(sp.out_scores_, res.scores.size() * 4, err)) return -3;
    if (search_device(d, sp, nq, d_q, kq, d_qids, d_qw, w_dense, w_sparse, nullptr, k, sp.out_ids_.as<int32_t>(), sp.out_scores_.as<float>(), s, err, inverted) != 0) {
        (void)hipStreamSynchronize(s);
        return -3;
    }
    if (!sp.results_to_host(s, 0, res.ids.size(), res, err)) return -3;
    res.deliver(ids, scores);
    return 0;
}

int Hybrid::search_host(Index &d, SparseIndex &sp, int nq, const float *q, int kq, const int32_t *qids, const float *qw, float w_dense,
                        float w_sparse, const uint32_t *allow, int k, int32_t *ids, float *scores, std::string &err, bool inverted) {
    if (nq <= 0) return 0;
    if (!sparse_queries_ok(nq, kq, qids, qw, sp.n_vocab_, err)) return -2;
    DeviceGuard g(sp.eng_->device());
    hipStream_t s = sp.stream_;
    // (the allow-list goes into the sparse index's buffer on its stream, behind whatever is queued on it)
    const uint32_t *d_allow = nullptr;
    if (!sp.upload_allow(allow, s, d_allow, err)) return -3;
    HostResults res((size_t)nq * k);
    const int dim = d.dim_;
    for (int c0 = 0; c0 < nq; c0 += Index::QCHUNK) {
        const int c = std::min(Index::QCHUNK, nq - c0);
        const size_t half = ((size_t)c * kq * 4 + 15) & ~(size_t)15;
        if (!d.grow(d.stage_, (size_t)c * dim * 4, err) || !sp.grow(sp.stage_, 2 * half, err) || !sp.grow(sp.out_ids_, (size_t)c * k * 4, err) ||
            !sp.grow(sp.out_scores_, (size_t)c * k * 4, err)) return -3;
        char *st = sp.stage_.as<char>();
        // (the staging buffers are the two indexes': behind both events)
        HIP_OK(hipStreamWaitEvent(s, sp.busy_, 0), err, -3);
        HIP_OK(hipStreamWaitEvent(s, d.busy_, 0), err, -3);
        HIP_OK(hipMemcpyAsync(d.stage_.p, q + (size_t)c0 * dim, (size_t)c * dim * 4, hipMemcpyHostToDevice, s), err, -3);
        HIP_OK(hipMemcpyAsync(st, qids + (size_t)c0 * kq, (size_t)c * kq * 4, hipMemcpyHostToDevice, s), err, -3);
        HIP_OK(hipMemcpyAsync(st + half, qw + (size_t)c0 * kq, (size_t)c * kq * 4, hipMemcpyHostToDevice, s), err, -3);
        if (search_device(d, sp, c, d.stage_.as<float>(), kq, (const int32_t *)st, (const float *)(st + half), w_dense, w_sparse, d_allow, k,
                          sp.out_ids_.as<int32_t>(), sp.out_scores_.as<float>(), s, err, inverted) != 0) {
            (void)hipStreamSynchronize(s);
            return -3;
        }
        if (!sp.results_to_host(s, (size_t)c0 * k, (size_t)c * k, res, err)) return -3;
    }
    res.deliver(ids, scores);
    return 0;
}

}  // namespace bert_hip
