// index.cpp — the host side of the embedding index (search.h): storage and its growth, add, the search, rescore, two-stage and
// probed routes, reading rows back, compaction, the file form (partition: index_partition.cpp; live bits, remove, stream and event: index_frame.h; file frame: index_io.h).  Kernels: search.hip behind search_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "index_io.h"
#include "search.h"
#include "search_kernels.h"

namespace bert_hip {

namespace {

// What the host knows of a row form, by dtype (the device's side of it: ScoreBlock<T> in search.hip; the bytes of a stored
// row: index_file.h).  The names are the profiler's; ingest is the kernel that makes the stored form of f32 rows.
struct FormInfo {
    const char *topk[2], *rescore, *probe, *probe_masked, *exported, *ingest;      // topk[1], probe_masked: the masked instantiations
    bool has_rscale;                             // one f32 scale per row beside the rows
    bool quantized_queries;                      // queries are stored as rows of the i8 form (codes and a scale), else of this one
};
constexpr FormInfo FORMS[4] = {
    {{"index_topk_f32", "index_topk_f32_masked"}, "index_rescore_f32", "index_probe_f32", "index_probe_f32_masked", "index_export_f32", "index_convert_f32", false, false},
    {{"index_topk_f16", "index_topk_f16_masked"}, "index_rescore_f16", "index_probe_f16", "index_probe_f16_masked", "index_export_f16", "index_convert_f16", false, false},
    {{"index_topk_i8", "index_topk_i8_masked"}, "index_rescore_i8", "index_probe_i8", "index_probe_i8_masked", "index_export_i8", "index_quantize_i8", true, true},
    {{"index_topk_b1", "index_topk_b1_masked"}, "index_rescore_b1", "index_probe_b1", "index_probe_b1_masked", "index_export_b1", "index_pack_b1", false, true},
};
int query_form(int dtype) { return FORMS[dtype].quantized_queries ? 2 : dtype; }

// slices of a search: enough workgroups to fill the chip, but each slice long against k (the first k rows of a slice all
// enter its list, and the merge reads slices x k candidates per query).  Grows with n_rows.
int slice_count(int n_rows, int nq, int k) {
    const int nqt = (nq + QT - 1) / QT, min_rows = std::max(2048, 16 * k);
    return std::max(1, std::min((TARGET_BLOCKS + nqt - 1) / nqt, n_rows / min_rows));
}

// (plan's slice count is at most slice_count; taken over every tile count and k' <= k by reserve)
size_t ws_entries_bound(int n_rows, int nq, int k) { return (size_t)nq * slice_count(n_rows, nq, k) * k; }

// how a chunk of nq queries is cut into workgroups of index_topk_kernel, and their LDS
struct Plan { int nqt, slices, slice_rows, L; size_t lds; };
Plan plan(int n_rows, int nq, int k) {
    Plan p;
    p.nqt = (nq + QT - 1) / QT;
    const int s = slice_count(n_rows, nq, k);
    const SliceCut c = slice_cut(n_rows, s, STEP_ROWS);
    p.slice_rows = c.rows; p.slices = c.n_slices;
    p.L = index_topk_L(k);
    p.lds = (size_t)std::min(QT, nq) * p.L * 8 + QT * 4;
    return p;
}

// The argument checks, one function per operation for its device and its host form: 1 = go on, 0 = nothing to do, -1 = err
int check_add(int n, const float *rows, int size, std::string &err) {
    if (n < 0 || (n > 0 && !rows)) { err = "add: n >= 0 and a row pointer required"; return -1; }
    if ((long long)size + n > INT_MAX) { err = "add: an index holds at most 2^31 - 1 rows"; return -1; }
    return n > 0;
}

int check_search(int nq, const void *q, int k, const void *ids, const void *scores, std::string &err) {
    if (k < 1 || k > Index::MAX_K) { err = "search: k must be 1 .. 256"; return -1; }
    if (nq < 0 || (nq > 0 && (!q || !ids || !scores))) { err = "search: n_queries >= 0 and query / result pointers required"; return -1; }
    return nq > 0;
}

int check_rescore(int nq, const void *q, int n_cand, const void *cand, int k, const void *ids, const void *scores, std::string &err) {
    if (k < 1 || k > Index::MAX_K) { err = "rescore: k must be 1 .. 256"; return -1; }
    if (n_cand < 1 || n_cand > Index::MAX_CAND) { err = "rescore: n_cand must be 1 .. 1024"; return -1; }
    if (nq < 0 || (nq > 0 && (!q || !cand || !ids || !scores))) { err = "rescore: n_queries >= 0 and query / candidate / result pointers required"; return -1; }
    return nq > 0;
}

int check_search_rescored(int nq, const void *q, int n_cand, int k, const void *ids, const void *scores, std::string &err) {
    if (n_cand < 1 || n_cand > Index::MAX_K || k < 1 || k > n_cand) { err = "search_rescored: 1 <= k <= n_cand <= 256 required"; return -1; }
    if (nq < 0 || (nq > 0 && (!q || !ids || !scores))) { err = "search_rescored: n_queries >= 0 and query / result pointers required"; return -1; }
    return nq > 0;
}

}  // namespace

void index_search_plan(int n_rows, int nq, int k, int geometry[4]) {
    const Plan p = plan(n_rows, nq, k);
    geometry[0] = p.nqt; geometry[1] = p.slices; geometry[2] = p.slice_rows; geometry[3] = p.L;
}

Index *Index::create(Engine *eng, int dim, int dtype, std::string &err) {
    if (!eng) { err = "no device engine"; return nullptr; }
    if (dim < 1 || dim > MAX_DIM) { err = "dim must be 1 .. 2048"; return nullptr; }
    if (dtype < 0 || dtype > 3) { err = "dtype must be 0 (f32), 1 (f16), 2 (i8) or 3 (b1)"; return nullptr; }
    DeviceGuard g(eng->device());
    Index *ix = new Index;
    ix->dim_ = dim;
    ix->dtype_ = dtype;
    // the score kernel's k-step (a 16-byte load per lane)
    ix->dpad_ = index_dpad(dtype, dim);
    ix->row_bytes_ = (size_t)index_row_bytes(dtype, ix->dpad_);
    ix->qrow_bytes_ = (size_t)index_row_bytes(query_form(dtype), ix->dpad_);
    if (!ix->open(eng, "index", err)) { delete ix; return nullptr; }
    search_kernels_init();
    return ix;
}

Index::~Index() {
    DeviceGuard g(eng_ ? eng_->device() : 0);
    close();
    if (rows_) (void)hipFree(rows_);
    if (rscale_) (void)hipFree(rscale_);
}

bool Index::grow_rows(int n_rows, std::string &err) {
    if (n_rows <= cap_) return true;
    const int cap = (int)std::min<long long>(INT_MAX, std::max<long long>({(long long)n_rows, (long long)cap_ * 3 / 2, 1024}));
    const size_t row_bytes = row_bytes_;
    void *p = nullptr;
    float *sc = nullptr;
    HIP_OK(hipEventSynchronize(busy_), err, false);
    HIP_OK(hipMalloc(&p, (size_t)cap * row_bytes), err, false);
    if (FORMS[dtype_].has_rscale && hipMalloc(&sc, (size_t)cap * 4) != hipSuccess) {
        (void)hipFree(p);
        err = "hipMalloc (index row scales) failed";
        return false;
    }
    // (an index with removed rows: the live words grow with the rows, so that an add within the capacity never allocates)
    uint32_t *lv = nullptr;
    bool ok = live_for_capacity(cap, lv, err);
    if (ok && n_ > 0 && hipMemcpy(p, rows_, (size_t)n_ * row_bytes, hipMemcpyDeviceToDevice) != hipSuccess) { err = "hipMemcpy (index rows) failed"; ok = false; }
    if (ok && n_ > 0 && sc && hipMemcpy(sc, rscale_, (size_t)n_ * 4, hipMemcpyDeviceToDevice) != hipSuccess) { err = "hipMemcpy (index row scales) failed"; ok = false; }
    if (!ok) {
        (void)hipFree(p);
        if (sc) (void)hipFree(sc);
        if (lv) (void)hipFree(lv);
        return false;
    }
    if (rows_) (void)hipFree(rows_);
    if (rscale_) (void)hipFree(rscale_);
    adopt_live(lv, cap);
    rows_ = p;
    rscale_ = sc;
    cap_ = cap;
    return true;
}

bool Index::reserve(int n_rows, int n_queries, int k, std::string &err) {
    if (n_rows < 0 || n_queries < 0 || k < 1 || k > MAX_K) { err = "reserve: n_rows, n_queries >= 0 and 1 <= k <= 256 required"; return false; }
    DeviceGuard g(eng_->device());
    if (!grow_rows(n_rows, err)) return false;
    const int nqc = std::min(n_queries, QCHUNK);
    if (nqc == 0) return true;
    size_t ent = 0;
    const int rows = std::max(n_rows, n_);
    for (int kk = 1; kk <= k; ++kk)
        for (int t = 1; t <= (nqc + QT - 1) / QT; ++t) ent = std::max(ent, ws_entries_bound(rows, std::min(nqc, t * QT), kk));
    return grow(ws_s_, ent * 4, err) && grow(ws_i_, ent * 4, err) && grow_queries(nqc, err);
}

// the stored form of a chunk of nqc queries (quantized: codes and scales)
bool Index::grow_queries(int nqc, std::string &err) {
    return grow(qbuf_, (size_t)nqc * qrow_bytes_, err) && (!FORMS[dtype_].quantized_queries || grow(qscale_, (size_t)nqc * 4, err));
}

int Index::add_device(int n, const float *d_rows, hipStream_t s, std::string &err) {
    if (const int go = check_add(n, d_rows, n_, err); go <= 0) return go < 0 ? -1 : n_;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;                                     // (engine.h: the one-event rule, and what a capturing stream changes)
    if (!eng_->op_begin(s, busy_, op, err)) return -1;
    if (!grow_rows(n_ + n, err)) return -1;
    char *dst = (char *)rows_ + (size_t)n_ * row_bytes_;
    eng_->timed_launch(FORMS[dtype_].ingest, 0.0, s, [&] { launch_ingest(dtype_, d_rows, dst, rscale_ ? rscale_ + n_ : nullptr, n, dim_, dpad_, s); });
    // (rows added after a removal are live: their bits on the same stream, and in the mirror, which is already long enough)
    if (live_) launch_live_set_range(live_, n_, n, s);
    HIP_OK(hipGetLastError(), err, -1);
    if (!eng_->op_end(op, err)) return -1;
    if (live_) bits_.set_range(n_, n);
    const int first = n_;
    n_ += n;
    return first;
}

int Index::add_host(int n, const float *rows, std::string &err) {
    if (const int go = check_add(n, rows, n_, err); go <= 0) return go < 0 ? -1 : n_;
    DeviceGuard g(eng_->device());
    const int first = n_;
    if (!grow_rows(n_ + n, err)) return -1;
    // through a staging buffer of at most 64 MiB (a row's stored form does not depend on the parts it came in)
    const int per = (int)std::max<size_t>(1, ((size_t)64 << 20) / ((size_t)dim_ * 4));
    for (int i0 = 0; i0 < n; i0 += per) {
        const int c = std::min(per, n - i0);
        if (!grow(stage_, (size_t)c * dim_ * 4, err) ||
            hipMemcpyAsync(stage_.p, rows + (size_t)i0 * dim_, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            add_device(c, stage_.as<float>(), stream_, err) < 0 || hipStreamSynchronize(stream_) != hipSuccess) {
            (void)hipStreamSynchronize(stream_);
            if (err.empty()) err = "add: copy to the device failed";
            truncate(first);
            return -1;
        }
    }
    return first;
}

// f32 queries -> qbuf_ (and qscale_) in the form the score block reads: the rows', or i8 codes padded to this dpad and their scales
void Index::enqueue_queries(int nq, const float *d_q, hipStream_t s) {
    const int form = query_form(dtype_);
    eng_->timed_launch(FORMS[form].ingest, 0.0, s, [&] { launch_ingest(form, d_q, qbuf_.p, qscale_.as<float>(), nq, dim_, dpad_, s); });
}

void Index::enqueue_chunk(int nq, const float *d_q, int k, int32_t *d_ids, float *d_scores, hipStream_t s, const uint32_t *d_allow) {
    const Plan p = plan(n_, nq, k);
    enqueue_queries(nq, d_q, s);
    TopkArgs a;
    a.rows = rows_; a.queries = qbuf_.p; a.qscale = qscale_.as<float>(); a.rscale = rscale_;
    a.live = live_; a.allow = d_allow;                       // (removed rows or an allow-list: the masked kernel, the same plan and workspace)
    a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
    a.n_rows = n_; a.dpad = dpad_; a.nq = nq; a.n_qtiles = p.nqt; a.n_slices = p.slices; a.slice_rows = p.slice_rows;
    a.k = k; a.L = p.L; a.n_items = p.nqt * p.slices;
    eng_->timed_launch(FORMS[dtype_].topk[live_ || d_allow], 2.0 * nq * (double)n_ * dim_, s, [&] { launch_topk(dtype_, a, p.lds, s); });
    enqueue_merge(nq, p.slices * k, k, d_ids, d_scores, s);
}

int Index::search_device(int nq, const float *d_q, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                         const uint32_t *d_allow) {
    if (const int go = check_search(nq, d_q, k, d_ids, d_scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -1;
    const int nqc = std::min(nq, QCHUNK);
    // (the last, shorter chunk may be cut into more slices than a full one)
    const size_t ent = std::max(ws_entries_bound(n_, nqc, k), nq % QCHUNK ? ws_entries_bound(n_, nq % QCHUNK, k) : 0);
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow_queries(nqc, err)) return -1;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        enqueue_chunk(c, d_q + (size_t)c0 * dim_, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s, d_allow);
    }
    HIP_OK(hipGetLastError(), err, -1);
    return eng_->op_end(op, err) ? 0 : -1;
}

// The loop of the host routes, blocking: per chunk of QCHUNK queries, the queries into stage_ (unless they are on the device;
// wait: behind the event, for the routes whose device form does not start with that wait), device_form(c0, c, d_q, d_ids,
// d_scores) on stream_, which may stage more of its own, and the results back.  A failed device form is synchronised with
// before the error returns; ids and scores are written only on success.
int Index::host_route(int nq, const float *q, bool q_on_device, bool wait, int k, int32_t *ids, float *scores, std::string &err,
                      const std::function<int(int, int, const float *, int32_t *, float *)> &device_form) {
    HostResults res((size_t)nq * k);
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const float *dq = q + (size_t)c0 * dim_;
        if (!q_on_device && !grow(stage_, (size_t)c * dim_ * 4, err)) return -1;
        if (!grow(out_ids_, (size_t)c * k * 4, err) || !grow(out_scores_, (size_t)c * k * 4, err)) return -1;
        if (wait) HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -1);
        if (!q_on_device) {
            HIP_OK(hipMemcpyAsync(stage_.p, dq, (size_t)c * dim_ * 4, hipMemcpyHostToDevice, stream_), err, -1);
            dq = stage_.as<float>();
        }
        if (device_form(c0, c, dq, out_ids_.as<int32_t>(), out_scores_.as<float>()) != 0) { (void)hipStreamSynchronize(stream_); return -1; }
        if (!results_to_host(stream_, (size_t)c0 * k, (size_t)c * k, res, err)) return -1;
    }
    res.deliver(ids, scores);
    return 0;
}

int Index::search_to_host(int nq, const float *q, bool q_on_device, int k, int32_t *ids, float *scores, std::string &err,
                          const uint32_t *allow) {
    if (const int go = check_search(nq, q, k, ids, scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    const uint32_t *d_allow = nullptr;
    if (!upload_allow(allow, stream_, d_allow, err)) return -1;
    return host_route(nq, q, q_on_device, false, k, ids, scores, err, [&](int, int c, const float *d_q, int32_t *d_ids, float *d_scores) {
        return search_device(c, d_q, k, d_ids, d_scores, stream_, err, d_allow);
    });
}

// ------------------------------------------------------------------------------------------------
// rescoring, two-stage search
// ------------------------------------------------------------------------------------------------
int Index::rescore_device(int nq, const float *d_q, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids, float *d_scores,
                          hipStream_t s, std::string &err) {
    if (const int go = check_rescore(nq, d_q, n_cand, d_cand, k, d_ids, d_scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -1;
    const int nqc = std::min(nq, QCHUNK);
    const size_t ent = (size_t)nqc * n_cand;
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow_queries(nqc, err)) return -1;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        enqueue_queries(c, d_q + (size_t)c0 * dim_, s);
        RescoreArgs a;
        a.rows = rows_; a.queries = qbuf_.p; a.qscale = qscale_.as<float>(); a.rscale = rscale_; a.live = live_;
        a.cand = d_cand + (size_t)c0 * n_cand; a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
        a.n_rows = n_; a.dpad = dpad_; a.nq = c; a.n_cand = n_cand; a.n_blocks = (n_cand + 31) / 32;
        eng_->timed_launch(FORMS[dtype_].rescore, 2.0 * c * (double)n_cand * dim_, s, [&] { launch_rescore(dtype_, a, s); });
        enqueue_merge(c, n_cand, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
    }
    HIP_OK(hipGetLastError(), err, -1);
    return eng_->op_end(op, err) ? 0 : -1;
}

int Index::rescore_to_host(int nq, const float *q, int n_cand, const int32_t *cand, int k, int32_t *ids, float *scores, std::string &err) {
    if (const int go = check_rescore(nq, q, n_cand, cand, k, ids, scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    return host_route(nq, q, false, true, k, ids, scores, err, [&](int c0, int c, const float *d_q, int32_t *d_ids, float *d_scores) {
        if (!grow(cand_in_, (size_t)c * n_cand * 4, err)) return -1;
        HIP_OK(hipMemcpyAsync(cand_in_.p, cand + (size_t)c0 * n_cand, (size_t)c * n_cand * 4, hipMemcpyHostToDevice, stream_), err, -1);
        return rescore_device(c, d_q, n_cand, cand_in_.as<int32_t>(), k, d_ids, d_scores, stream_, err);
    });
}

int Index::search_rescored_device(Index &coarse, int nq, const float *d_q, int n_cand, int k, int32_t *d_ids, float *d_scores,
                                  hipStream_t s, std::string &err, int nprobe, const uint32_t *d_allow) {
    if (const int go = check_search_rescored(nq, d_q, n_cand, k, d_ids, d_scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    // (the candidate lists are this index's: the coarse search that fills them waits for whatever still reads them; after
    // that the two steps of a chunk, and the chunks, follow each other on s.  The rescore of each chunk ends the operation.)
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -1;
    const int nqc = std::min(nq, QCHUNK);
    if (!grow(cand_i_, (size_t)nqc * n_cand * 4, err) || !grow(cand_s_, (size_t)nqc * n_cand * 4, err)) return -1;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const float *dq = d_q + (size_t)c0 * dim_;
        const int r = nprobe > 0 ? coarse.search_probed_device(c, dq, nprobe, n_cand, cand_i_.as<int32_t>(), cand_s_.as<float>(), s, err, d_allow)
                                 : coarse.search_device(c, dq, n_cand, cand_i_.as<int32_t>(), cand_s_.as<float>(), s, err);
        if (r != 0) return -1;
        if (rescore_device(c, dq, n_cand, cand_i_.as<int32_t>(), k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s, err) != 0) return -1;
    }
    return 0;
}

int Index::search_rescored_to_host(Index &coarse, int nq, const float *q, int n_cand, int k, int32_t *ids, float *scores, std::string &err,
                                   int nprobe, const uint32_t *allow) {
    if (const int go = check_search_rescored(nq, q, n_cand, k, ids, scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    // (the list goes into coarse's buffer on this index's stream, on which coarse's searches follow)
    const uint32_t *d_allow = nullptr;
    if (nprobe > 0 && !coarse.upload_allow(allow, stream_, d_allow, err)) return -1;
    return host_route(nq, q, false, true, k, ids, scores, err, [&](int, int c, const float *d_q, int32_t *d_ids, float *d_scores) {
        return search_rescored_device(coarse, c, d_q, n_cand, k, d_ids, d_scores, stream_, err, nprobe, d_allow);
    });
}

// ------------------------------------------------------------------------------------------------
// probed search (the partition: index_partition.cpp), rows read back
// ------------------------------------------------------------------------------------------------
int Index::search_probed_device(int nq, const float *d_q, int nprobe, int k, int32_t *d_ids, float *d_scores, hipStream_t s, std::string &err,
                                const uint32_t *d_allow) {
    if (const int go = check_search(nq, d_q, k, d_ids, d_scores, err); go <= 0) return go;
    if (!cent_ || nprobe < 1 || nprobe > std::min(n_lists(), MAX_K)) { err = "search_probed: a partition and 1 <= nprobe <= min(n_lists, 256) required"; return -1; }
    DeviceGuard g(eng_->device());
    // (the probe lists are this index's: the centroid search that fills them waits, on s, for whatever still reads them)
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -1;
    const int nqc = std::min(nq, QCHUNK);
    // items per query: the probed lists, then the chunks of the tail
    const int n_items = nprobe + (int)(((long long)n_ - n_part_ + PROBE_CHUNK - 1) / PROBE_CHUNK);
    const size_t ent = (size_t)nqc * n_items * k;
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow_queries(nqc, err) ||
        !grow(probe_i_, (size_t)nqc * nprobe * 4, err) || !grow(probe_s_, (size_t)nqc * nprobe * 4, err)) return -1;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        const float *dq = d_q + (size_t)c0 * dim_;
        if (cent_->search_device(c, dq, nprobe, probe_i_.as<int32_t>(), probe_s_.as<float>(), s, err) != 0) return -1;
        enqueue_queries(c, dq, s);
        ProbeArgs a;
        a.rows = rows_; a.queries = qbuf_.p; a.qscale = qscale_.as<float>(); a.rscale = rscale_; a.live = live_;
        a.probe = probe_i_.as<int32_t>(); a.offsets = offsets_.as<int32_t>(); a.order = order_.as<int32_t>();
        a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
        a.n_rows = n_; a.dpad = dpad_; a.nq = c; a.nprobe = nprobe; a.n_lists = n_lists(); a.n_part = n_part_; a.n_items = n_items;
        a.k = k; a.L = probe_L(k);
        a.allow = d_allow;                                   // (an allow-list: the masked kernel, the same items and workspace)
        eng_->timed_launch(d_allow ? FORMS[dtype_].probe_masked : FORMS[dtype_].probe, 0.0, s, [&] { launch_probe(dtype_, a, s); });
        enqueue_merge(c, n_items * k, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
    }
    HIP_OK(hipGetLastError(), err, -1);
    return eng_->op_end(op, err) ? 0 : -1;
}

int Index::search_probed_to_host(int nq, const float *q, int nprobe, int k, int32_t *ids, float *scores, std::string &err,
                                 const uint32_t *allow) {
    if (const int go = check_search(nq, q, k, ids, scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    const uint32_t *d_allow = nullptr;
    if (!upload_allow(allow, stream_, d_allow, err)) return -1;
    return host_route(nq, q, false, true, k, ids, scores, err, [&](int, int c, const float *d_q, int32_t *d_ids, float *d_scores) {
        return search_probed_device(c, d_q, nprobe, k, d_ids, d_scores, stream_, err, d_allow);
    });
}

// rows ids[i] (d_ids null: first + i) as f32 into d_out [n][dim]
void Index::enqueue_export(int first, int n, const int32_t *d_ids, float *d_out, hipStream_t s) {
    ExportArgs a;
    a.rows = rows_; a.rscale = rscale_; a.ids = d_ids; a.out = d_out; a.first = first; a.n = n; a.dim = dim_; a.dpad = dpad_;
    eng_->timed_launch(FORMS[dtype_].exported, 0.0, s, [&] { launch_export(dtype_, a, s); });
}

int Index::get_rows(int n, const int32_t *ids, float *rows, std::string &err) {
    if (n <= 0) return 0;
    DeviceGuard g(eng_->device());
    // through device buffers of at most 64 MiB, as add_host
    const int per = (int)std::max<size_t>(1, ((size_t)64 << 20) / ((size_t)dim_ * 4));
    for (int i0 = 0; i0 < n; i0 += per) {
        const int c = std::min(per, n - i0);
        if (!grow(cand_in_, (size_t)c * 4, err) || !grow(export_, (size_t)c * dim_ * 4, err)) return -1;
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -1);
        HIP_OK(hipMemcpyAsync(cand_in_.p, ids + i0, (size_t)c * 4, hipMemcpyHostToDevice, stream_), err, -1);
        enqueue_export(0, c, cand_in_.as<int32_t>(), export_.as<float>(), stream_);
        HIP_OK(hipGetLastError(), err, -1);
        HIP_OK(hipEventRecord(busy_, stream_), err, -1);
        HIP_OK(hipMemcpyAsync(rows + (size_t)i0 * dim_, export_.p, (size_t)c * dim_ * 4, hipMemcpyDeviceToHost, stream_), err, -1);
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// removed rows, compaction, file form
// ------------------------------------------------------------------------------------------------
void Index::truncate(int n) {
    if (n < 0 || n >= n_) return;
    if (live_) bits_.truncate(n_, n);                        // (live_bits.h: the mirror's side of the invariant; the device words stay)
    n_ = n;
}

int Index::remove(int n, const int32_t *ids, std::string &err) {
    std::vector<int32_t> fresh;                          // the ids this call removes (repeats and removed rows left out)
    return remove_rows(n, ids, cap_, fresh, err) == Removed::ok ? (int)fresh.size() : -1;
}

int Index::compact(int32_t *old_ids, std::string &err) {
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -1);
    if (bits_.n_removed == 0) return compact_nothing(old_ids);
    const std::vector<int32_t> map = bits_.kept(n_);
    const int nl = (int)map.size();
    const size_t row_bytes = row_bytes_;
    void *p = nullptr;
    float *sc = nullptr;
    int32_t *d_map = nullptr;
    const char *failed = nullptr;
    if (nl > 0) {
        if (hipMalloc(&p, (size_t)nl * row_bytes) != hipSuccess) failed = "hipMalloc (index rows) failed";
        else if (FORMS[dtype_].has_rscale && hipMalloc((void **)&sc, (size_t)nl * 4) != hipSuccess) failed = "hipMalloc (index row scales) failed";
        else if (hipMalloc((void **)&d_map, (size_t)nl * 4) != hipSuccess) failed = "hipMalloc (compaction ids) failed";
        else if (hipMemcpyAsync(d_map, map.data(), (size_t)nl * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) failed = "hipMemcpy (compaction ids) failed";
        else {
            eng_->timed_launch("index_gather", 0.0, stream_, [&] { launch_gather(rows_, p, rscale_, sc, d_map, nl, row_bytes, stream_); });
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) failed = "the gather kernel failed";
        }
        if (d_map) (void)hipFree(d_map);
        if (failed) {
            if (p) (void)hipFree(p);
            if (sc) (void)hipFree(sc);
            err = failed;
            return -1;
        }
    }
    if (rows_) (void)hipFree(rows_);
    if (rscale_) (void)hipFree(rscale_);
    rows_ = p;
    rscale_ = sc;
    cap_ = n_ = nl;
    drop_live();
    if (old_ids) memcpy(old_ids, map.data(), (size_t)nl * 4);
    if (cent_) {
        // the partition follows the rows: each keeps its list, and the tail (the old ids from n_part_ on) stays the tail
        std::vector<int32_t> kept;
        for (int32_t old : map)
            if (old < n_part_) kept.push_back(list_of_[(size_t)old]);
        if (!upload_lists(kept, n_lists(), err)) {
            drop_partition();
            err = "the rows are compacted, but the partition was dropped: " + err;
            return -1;
        }
        n_part_ = (int)kept.size();
        list_of_ = std::move(kept);
    }
    return nl;
}

// device memory <-> file in pieces of at most 64 MiB through a host buffer (index_io.h)
static constexpr size_t FILE_PIECE = (size_t)64 << 20;

bool Index::save(const char *path, std::string &err) {
    if (!path || !*path) { err = "a path is required"; return false; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, false);
    IndexFileHeader h;
    h.dtype = (uint32_t)dtype_; h.dim = (uint32_t)dim_; h.dpad = (uint32_t)dpad_; h.n_rows = (uint32_t)n_; h.has_live = live_ ? 1u : 0u;
    unsigned char hdr[INDEX_HEADER_BYTES];
    index_header_write(h, hdr);
    return write_atomically(path, err, [&](FILE *f) {
        std::vector<char> buf;
        // (the live words come from the mirror: its bits at and beyond size are zero)
        return fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr && device_to_file(f, rows_, (size_t)n_ * row_bytes_, FILE_PIECE, buf, err) &&
               (!FORMS[dtype_].has_rscale || device_to_file(f, rscale_, (size_t)n_ * 4, FILE_PIECE, buf, err)) &&
               (!live_ || fwrite(bits_.words.data(), 4, live_words(n_), f) == live_words(n_));
    });
}

bool Index::load_rows(FILE *f, const IndexFileHeader &h, std::string &err) {
    if (n_ != 0 || live_ || (int)h.dtype != dtype_ || (int)h.dim != dim_ || (int)h.dpad != dpad_) { err = "load: the index does not fit the file"; return false; }
    DeviceGuard g(eng_->device());
    const int n = (int)h.n_rows;
    if (!grow_rows(n, err)) return false;
    std::vector<char> buf;
    if (!file_to_device(f, rows_, (size_t)n * row_bytes_, FILE_PIECE, buf, err)) return false;
    if (FORMS[dtype_].has_rscale && !file_to_device(f, rscale_, (size_t)n * 4, FILE_PIECE, buf, err)) return false;
    n_ = n;
    if (!h.has_live) return true;
    std::vector<uint32_t> words(live_words(n));
    if (fread(words.data(), 4, words.size(), f) != words.size()) { n_ = 0; err = "read failed"; return false; }
    if (!install_live(words.data(), cap_, err)) { n_ = 0; return false; }
    return true;
}

float *Index::scratch(size_t n, std::string &err) {
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, nullptr);
    return scratch_.ensure(n * 4, err) ? scratch_.as<float>() : nullptr;
}

}  // namespace bert_hip
