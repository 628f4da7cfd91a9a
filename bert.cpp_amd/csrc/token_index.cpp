// token_index.cpp — the host side of the token index (token_index.h): storage and its growth, the add forms, the search and its
// chunks, rescoring, reading a document back, the checks of the host forms, compaction and the file form (live bits, remove, stream
// and event: index_frame.h; file frame: index_io.h).  Every kernel is in token_index.hip (both forms), maxsim.hip or search.hip (the merge, the live bits of added documents) and reached through
// token_index_kernels.h / kernels.h / search_kernels.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <vector>

#include <sys/types.h>

#include "index_io.h"
#include "search_kernels.h"
#include "token_index.h"

namespace bert_hip {

namespace {

// the most workspace entries (nq' * slices * k) a chunk of up to nqc queries takes: the slice count falls as the queries grow
size_t ws_entries_bound(int n_docs, int nqc, int k, int pref) {
    size_t ent = 0;
    TokenScanPlan p;
    for (int q = 1; q <= nqc; ++q)
        if (token_index_plan(n_docs, q, pref, p)) ent = std::max(ent, (size_t)q * p.max_slices * k);
    return ent;
}

// 1 = go on, 0 = nothing to do, -2 = refused
int check_add(int n_docs, const int32_t *cu, const void *rows, int size, int64_t n_tok, std::string &err) {
    if (n_docs < 0 || (n_docs > 0 && (!cu || !rows))) { err = "add: n_docs >= 0, cu and rows required"; return -2; }
    if (n_docs == 0) return 0;
    if (!token_cu_ok(cu, n_docs)) { err = "add: cu must ascend strictly from an entry >= 0 (every document has at least one token)"; return -2; }
    if ((long long)size + n_docs > INT_MAX - 1 || n_tok + ((long long)cu[n_docs] - cu[0]) > INT_MAX) { err = "add: an index holds fewer than 2^31 documents and tokens"; return -2; }
    return 1;
}

int check_search(int nq, const void *qcu, const void *q, int k, const void *ids, const void *scores, std::string &err) {
    if (k < 1 || k > TokenIndex::MAX_K) { err = "search: k must be 1 .. 256"; return -2; }
    if (nq < 0 || (nq > 0 && (!qcu || !q || !ids || !scores))) { err = "search: n_queries >= 0 and query / result pointers required"; return -2; }
    return nq > 0;
}

int check_rescore(int nq, const void *qcu, const void *q, int n_cand, const void *cand, int k, const void *ids, const void *scores, std::string &err) {
    if (k < 1 || k > TokenIndex::MAX_K) { err = "rescore: k must be 1 .. 256"; return -2; }
    if (n_cand < 1 || n_cand > TokenIndex::MAX_CAND) { err = "rescore: n_cand must be 1 .. 1024"; return -2; }
    if (nq < 0 || (nq > 0 && (!qcu || !q || !cand || !ids || !scores))) { err = "rescore: n_queries >= 0 and query / candidate / result pointers required"; return -2; }
    return nq > 0;
}

}  // namespace

bool token_cu_ok(const int32_t *cu, int n) {
    bool ok = cu[0] >= 0;
    for (int i = 0; ok && i < n; ++i) ok = cu[i + 1] > cu[i];
    return ok;
}

TokenIndex *TokenIndex::create(Engine *eng, int dim, int dtype, std::string &err) {
    if (!eng) { err = "no device engine"; return nullptr; }
    if (dim < 8 || dim > MAXSIM_MAX_H || dim % 8) { err = "dim must be a multiple of 8 in 8 .. " + std::to_string(MAXSIM_MAX_H); return nullptr; }
    if (dtype != 1 && dtype != 2) { err = "dtype must be 1 (f16) or 2 (int8)"; return nullptr; }
    DeviceGuard g(eng->device());
    TokenIndex *ix = new TokenIndex;
    ix->dim_ = dim;
    ix->dtype_ = dtype;
    ix->dpad_ = token_i8_dpad(dim);
    ix->cu_h_.assign(1, 0);
    if (!ix->open(eng, "token index", err)) { delete ix; return nullptr; }
    // (cu[0] = 0 is there from the start: an empty index is searched like any other)
    if (!ix->grow_storage(1, 0, err)) { delete ix; return nullptr; }
    token_index_kernels_init();
    return ix;
}

TokenIndex::~TokenIndex() {
    DeviceGuard g(eng_ ? eng_->device() : 0);
    close();
    if (rows_) (void)hipFree(rows_);
    if (scales_) (void)hipFree(scales_);
    if (cu_) (void)hipFree(cu_);
}

// (rows and cumulative lengths are plain arrays: growth is a copy each; the host mirror's capacity follows cu_'s, so that its
// entries never move while a copy from them may be queued)
bool TokenIndex::grow_storage(long long n_docs, long long n_tokens, std::string &err) {
    if (n_docs <= cap_docs_ && n_tokens <= cap_tok_) return true;
    HIP_OK(hipEventSynchronize(busy_), err, false);
    HIP_OK(hipStreamSynchronize(stream_), err, false);
    if (n_docs > cap_docs_) {
        const long long cap = std::min<long long>(INT_MAX - 1, std::max<long long>({n_docs, (long long)cap_docs_ * 3 / 2, 1024}));
        int32_t *pc = nullptr;
        // (an index with removed documents: the live words grow with the lengths, so that an add within the capacity never allocates)
        uint32_t *lv = nullptr;
        if (hipMalloc((void **)&pc, (size_t)(cap + 1) * 4) != hipSuccess) {
            (void)hipGetLastError();
            err = "hipMalloc (token index lengths) failed";
            return false;
        }
        if (hipMemcpy(pc, cu_h_.data(), (size_t)(n_ + 1) * 4, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(pc);
            err = "hipMemcpy (token index lengths) failed";
            return false;
        }
        if (!live_for_capacity(cap, lv, err)) { (void)hipFree(pc); return false; }
        if (cu_) (void)hipFree(cu_);
        cu_ = pc;
        adopt_live(lv, cap);
        cap_docs_ = (int)cap;
        cu_h_.reserve((size_t)cap + 1);
    }
    if (n_tokens > cap_tok_) {
        const long long cap = std::min<long long>(INT_MAX, std::max<long long>({n_tokens, (long long)cap_tok_ * 3 / 2, 4096}));
        char *pr = nullptr;
        float *ps = nullptr;                                 // (the int8 form's scales grow with its codes)
        const size_t row_bytes = this->row_bytes();
        if (hipMalloc((void **)&pr, (size_t)cap * row_bytes) != hipSuccess || (dtype_ == 2 && hipMalloc((void **)&ps, (size_t)cap * 4) != hipSuccess)) {
            (void)hipGetLastError();
            if (pr) (void)hipFree(pr);
            err = "hipMalloc (token index rows) failed";
            return false;
        }
        if (n_tok_ > 0 && (hipMemcpy(pr, rows_, (size_t)n_tok_ * row_bytes, hipMemcpyDeviceToDevice) != hipSuccess ||
                           (ps && hipMemcpy(ps, scales_, (size_t)n_tok_ * 4, hipMemcpyDeviceToDevice) != hipSuccess))) {
            (void)hipGetLastError();
            (void)hipFree(pr);
            if (ps) (void)hipFree(ps);
            err = "hipMemcpy (token index rows) failed";
            return false;
        }
        if (rows_) (void)hipFree(rows_);
        if (scales_) (void)hipFree(scales_);
        rows_ = pr;
        scales_ = ps;
        cap_tok_ = cap;
    }
    return true;
}

bool TokenIndex::grow_search(int n_docs, int nqc, int k, std::string &err) {
    const size_t ent = ws_entries_bound(n_docs, nqc, k, eng_->options().token_index_slices);
    return grow(ws_s_, ent * 4, err) && grow(ws_i_, ent * 4, err);
}

bool TokenIndex::grow_queries(int nqc, int max_q_len, std::string &err) {
    const size_t slots = (size_t)nqc * max_q_len;
    return grow(q_codes_, slots * dpad_, err) && grow(q_scales_, slots * 4, err);
}

void TokenIndex::quantize_rows(const void *d_src, bool src_f32, long long n, long long at, hipStream_t s) {
    TokenI8QuantizeArgs qa{d_src, (int8_t *)rows_ + (size_t)at * dpad_, scales_ + at, n, dim_, dpad_};
    eng_->timed_launch("token_i8_quantize", 0.0, s, [&] { launch_token_i8_quantize(qa, src_f32, s); });
}

int TokenIndex::reserve(int n_docs, int64_t n_tokens, int n_queries, int max_q_len, int k, std::string &err) {
    if (n_docs < 0 || n_tokens < 0 || n_tokens > INT_MAX || n_queries < 0 || k < 1 || k > MAX_K || max_q_len < 0 || max_q_len > max_query_tokens()) {
        err = "reserve: n_docs, n_queries >= 0, 0 <= n_tokens < 2^31, 1 <= k <= 256 and 0 <= max_q_len <= " + std::to_string(max_query_tokens()) + " required";
        return -2;
    }
    DeviceGuard g(eng_->device());
    if (!grow_storage(n_docs, n_tokens, err)) return -3;
    const int nqc = std::min(n_queries, QCHUNK);
    if (nqc == 0) return 0;
    if (dtype_ == 2 && !grow_queries(nqc, max_q_len, err)) return -3;
    return grow_search(std::max(n_docs, n_), nqc, k, err) ? 0 : -3;
}

bool TokenIndex::commit(int n_docs, const int32_t *cu, hipStream_t s, std::string &err) {
    const size_t at = cu_h_.size();                          // == n_ + 1 (the capacity is grow_storage's: no entry moves)
    for (int i = 1; i <= n_docs; ++i) cu_h_.push_back((int32_t)(n_tok_ + ((long long)cu[i] - cu[0])));
    if (hipMemcpyAsync(cu_ + at, cu_h_.data() + at, (size_t)n_docs * 4, hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        cu_h_.resize(at);
        err = "hipMemcpyAsync (token index lengths) failed";
        return false;
    }
    // (documents added after a removal are live: their bits on the same stream, and in the mirror, which is as long as the capacity)
    if (live_) {
        launch_live_set_range(live_, n_, n_docs, s);
        if (hipGetLastError() != hipSuccess) { cu_h_.resize(at); err = "the live bits of the new documents could not be set"; return false; }
        bits_.set_range(n_, n_docs);
    }
    n_ += n_docs;
    n_tok_ = cu_h_.back();
    return true;
}

int TokenIndex::add_device(int n_docs, const int32_t *cu, const half_t *d_rows, hipStream_t s, std::string &err) {
    if (const int go = check_add(n_docs, cu, d_rows, n_, n_tok_, err); go <= 0) return go < 0 ? go : n_;
    if ((uintptr_t)d_rows & 15) { err = "add: the rows must be 16-byte aligned"; return -2; }
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;                                     // (engine.h: the one-event rule)
    if (!eng_->op_begin(s, busy_, op, err)) return -3;
    const long long T = (long long)cu[n_docs] - cu[0];
    if (!grow_storage((long long)n_ + n_docs, n_tok_ + T, err)) return -3;
    if (dtype_ == 2) {
        quantize_rows(d_rows + (size_t)cu[0] * dim_, false, T, n_tok_, s);
        HIP_OK(hipGetLastError(), err, -3);
    } else {
        HIP_OK(hipMemcpyAsync(rows_ + (size_t)n_tok_ * row_bytes(), d_rows + (size_t)cu[0] * dim_, (size_t)T * dim_ * 2, hipMemcpyDeviceToDevice, s), err, -3);
    }
    const int first = n_;
    if (!commit(n_docs, cu, s, err)) return -3;
    if (!eng_->op_end(op, err)) return -3;
    return first;
}

int TokenIndex::add_host(int n_docs, const int32_t *cu, const float *rows, std::string &err) {
    if (const int go = check_add(n_docs, cu, rows, n_, n_tok_, err); go <= 0) return go < 0 ? go : n_;
    DeviceGuard g(eng_->device());
    const long long T = (long long)cu[n_docs] - cu[0];
    if (!grow_storage((long long)n_ + n_docs, n_tok_ + T, err)) return -3;
    // through a staging buffer of at most 32 MiB (a row's stored bits do not depend on the parts it came in; a part is at most 2^23
    // values or one row: far below F32_TO_F16_MAX_N)
    const long long per = std::max<long long>(1, ((long long)32 << 20) / ((long long)dim_ * 4));
    if (!grow(stage_, (size_t)std::min(per, T) * dim_ * 4, err)) return -3;
    Engine::StreamOp op;
    if (!eng_->op_begin(stream_, busy_, op, err)) return -3;
    for (long long t0 = 0; t0 < T; t0 += per) {
        const size_t c = (size_t)std::min(per, T - t0);
        bool ok = hipMemcpyAsync(stage_.p, rows + (size_t)(cu[0] + t0) * dim_, c * dim_ * 4, hipMemcpyHostToDevice, stream_) == hipSuccess;
        if (ok && dtype_ == 2) quantize_rows(stage_.p, true, (long long)c, n_tok_ + t0, stream_);
        else if (ok) eng_->timed_launch("f32_to_f16", 0.0, stream_, [&] { launch_f32_to_f16(stage_.as<float>(), (half_t *)rows_ + (size_t)(n_tok_ + t0) * dim_, c * dim_, stream_); });
        ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(stream_) == hipSuccess;
        if (!ok) { (void)hipStreamSynchronize(stream_); err = "add: copy to the device failed"; return -3; }
    }
    const int first = n_;
    if (!commit(n_docs, cu, stream_, err)) return -3;
    if (!eng_->op_end(op, err)) return -3;
    HIP_OK(hipStreamSynchronize(stream_), err, -3);
    return first;
}

half_t *TokenIndex::append_room(int64_t n_tokens, std::string &err) {
    if (n_tokens < 0 || n_tok_ + n_tokens > INT_MAX) { err = "add: an index holds fewer than 2^31 tokens"; return nullptr; }
    if (!grow_storage(n_, n_tok_ + n_tokens, err)) return nullptr;
    if (dtype_ == 2) return grow(text_rows_, std::max<size_t>((size_t)n_tokens * dim_ * 2, 16), err) ? text_rows_.as<half_t>() : nullptr;
    return (half_t *)rows_ + (size_t)n_tok_ * dim_;
}

int TokenIndex::add_in_place(int n_docs, const int32_t *cu, std::string &err) {
    if (const int go = check_add(n_docs, cu, rows_, n_, n_tok_, err); go <= 0) return go < 0 ? go : n_;
    if (cu[0] != 0 || n_tok_ + cu[n_docs] > cap_tok_) { err = "add: the rows in place do not match the room asked for"; return -2; }
    DeviceGuard g(eng_->device());
    // (the lengths first: growing them keeps rows_ and what the caller enqueued into it)
    if (!grow_storage((long long)n_ + n_docs, n_tok_, err)) return -3;
    Engine::StreamOp op;
    if (!eng_->op_begin(stream_, busy_, op, err)) return -3;
    if (dtype_ == 2) {
        // (the chunk's f16 rows wait in append_room's buffer, enqueued on stream() in front of this)
        if ((size_t)cu[n_docs] * dim_ * 2 > text_rows_.bytes) { err = "add: the rows in place do not match the room asked for"; return -2; }
        quantize_rows(text_rows_.p, false, cu[n_docs], n_tok_, stream_);
        HIP_OK(hipGetLastError(), err, -3);
    }
    const int first = n_;
    if (!commit(n_docs, cu, stream_, err)) return -3;
    if (!eng_->op_end(op, err)) return -3;
    return first;
}

void TokenIndex::truncate(int n) {
    if (n < 0 || n >= n_) return;
    // (after a failure, behind a synchronised stream: no copy from the mirror is queued)
    // (live_bits.h: the mirror's side of the invariant; the device words stay)
    if (live_) bits_.truncate(n_, n, [&](int d) { tok_removed_ -= cu_h_[(size_t)d + 1] - cu_h_[(size_t)d]; });
    cu_h_.resize((size_t)n + 1);
    n_ = n;
    n_tok_ = cu_h_.back();
}

int TokenIndex::get_doc(int id, float *rows, int cap_tokens, std::string &err) {
    if (id < 0 || id >= n_) { err = "get_doc: id " + std::to_string(id) + " outside [0, " + std::to_string(n_) + ")"; return -2; }
    const int len = cu_h_[(size_t)id + 1] - cu_h_[(size_t)id];
    if (!rows || cap_tokens < len) return len;
    DeviceGuard g(eng_->device());
    if (dtype_ == 2) {
        std::vector<int8_t> codes((size_t)len * dpad_);
        std::vector<float> sc((size_t)len);
        if (const int r = get_codes(id, codes.data(), sc.data(), len, err); r < 0) return r;
        for (int t = 0; t < len; ++t)
            for (int e = 0; e < dim_; ++e) rows[(size_t)t * dim_ + e] = (float)codes[(size_t)t * dpad_ + e] * sc[(size_t)t];
        return len;
    }
    std::vector<half_t> h((size_t)len * dim_);
    HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -3);
    HIP_OK(hipMemcpyAsync(h.data(), (const half_t *)rows_ + (size_t)cu_h_[(size_t)id] * dim_, h.size() * 2, hipMemcpyDeviceToHost, stream_), err, -3);
    HIP_OK(hipStreamSynchronize(stream_), err, -3);
    for (size_t i = 0; i < h.size(); ++i) rows[i] = (float)h[i];
    return len;
}

int TokenIndex::get_codes(int id, int8_t *codes, float *scales, int cap_tokens, std::string &err) {
    if (dtype_ != 2) { err = "get_codes: the index holds f16 rows (dtype 1), not int8 codes"; return -2; }
    if (id < 0 || id >= n_) { err = "get_codes: id " + std::to_string(id) + " outside [0, " + std::to_string(n_) + ")"; return -2; }
    const int t0 = cu_h_[(size_t)id], len = cu_h_[(size_t)id + 1] - t0;
    if (!codes || !scales || cap_tokens < len) return len;
    DeviceGuard g(eng_->device());
    HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -3);
    HIP_OK(hipMemcpyAsync(codes, rows_ + (size_t)t0 * dpad_, (size_t)len * dpad_, hipMemcpyDeviceToHost, stream_), err, -3);
    HIP_OK(hipMemcpyAsync(scales, scales_ + t0, (size_t)len * 4, hipMemcpyDeviceToHost, stream_), err, -3);
    HIP_OK(hipStreamSynchronize(stream_), err, -3);
    return len;
}

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
int TokenIndex::search_device(int nq, const int32_t *d_qcu, const half_t *d_q, int max_q_len, int k, int32_t *d_ids, float *d_scores, hipStream_t s,
                              std::string &err, const uint32_t *d_allow) {
    return search_any(nq, d_qcu, d_q, false, max_q_len, k, d_ids, d_scores, s, err, d_allow);
}

int TokenIndex::search_any(int nq, const int32_t *d_qcu, const void *d_q, bool q_f32, int max_q_len, int k, int32_t *d_ids, float *d_scores,
                           hipStream_t s, std::string &err, const uint32_t *d_allow) {
    if (const int go = check_search(nq, d_qcu, d_q, k, d_ids, d_scores, err); go <= 0) return go;
    if (max_q_len < 1 || max_q_len > max_query_tokens()) { err = "search: max_q_len must be 1 .. " + std::to_string(max_query_tokens()) + " at dim " + std::to_string(dim_); return -2; }
    if ((uintptr_t)d_q & 15) { err = "search: the query rows must be 16-byte aligned"; return -2; }
    return scan_chunks(nq, d_qcu, d_q, q_f32, max_q_len, k, d_ids, d_scores, s, err, d_allow, nullptr, 0);
}

// The chunk loop of every search and of the int8 rescore: per chunk of up to QCHUNK queries the plan, the int8 form's queries into the
// workspace (the kernel applies the scan's guards to d_qcu), the scan and the merge of the slices' lists.  A search (d_cand null) scans
// the n_ documents under live_ / d_allow; a rescore scans the n_cand positions of each query's candidate list — the search's plan with
// n_cand in the documents' place — and tests live_ per id.  The workspace [nq][slices][k] grows by the same bound over either count
int TokenIndex::scan_chunks(int nq, const int32_t *d_qcu, const void *d_q, bool q_f32, int max_q_len, int k, int32_t *d_ids, float *d_scores,
                            hipStream_t s, std::string &err, const uint32_t *d_allow, const int32_t *d_cand, int n_cand) {
    const bool i8 = dtype_ == 2;
    const int n_list = d_cand ? n_cand : n_;
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -3;
    const int nqc = std::min(nq, QCHUNK), pref = eng_->options().token_index_slices;
    if (!grow_search(n_list, nqc, k, err)) return -3;
    if (i8 && !grow_queries(nqc, max_q_len, err)) return -3;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        TokenScanPlan p;
        token_index_plan(n_list, c, pref, p);                 // (the key's range is the option's: never refused)
        TokenScanArgs a;
        a.rows = rows_; a.cu = cu_; a.q = d_q; a.qcu = d_qcu + c0; a.ws_s = ws_s_.as<float>(); a.ws_i = ws_i_.as<int>();
        a.n_docs = n_; a.dim = dim_; a.dpad = dpad_; a.nq = c; a.max_q_len = max_q_len; a.n_slices = p.n_slices; a.slice_docs = p.slice_docs;
        a.k = k; a.L = token_list_L(k); a.n_items = c * p.n_slices;
        if (i8) {
            TokenI8QuantizeArgs qa{d_q, q_codes_.as<int8_t>(), q_scales_.as<float>(), (long long)c * max_q_len, dim_, dpad_, d_qcu + c0, max_q_len};
            eng_->timed_launch("token_i8_quantize", 0.0, s, [&] { launch_token_i8_quantize(qa, q_f32, s); });
            a.scales = scales_; a.q = q_codes_.p; a.q_scales = q_scales_.as<float>();
        }
        // (removed documents or an allow-list: the masked kernel, the same plan and workspace; an empty index has no words to read)
        if (d_cand) { a.live = live_; a.cand = d_cand + (size_t)c0 * n_cand; a.n_cand = n_cand; }
        else if (n_ > 0) { a.live = live_; a.allow = d_allow; }
        const bool masked = a.live || a.allow;
        const char *label = d_cand ? "token_i8_rescore" : i8 ? (masked ? "token_i8_scan_masked" : "token_i8_scan") : (masked ? "token_index_scan_masked" : "token_index_scan");
        eng_->timed_launch(label, 0.0, s, [&] { launch_token_scan(dtype_, a, s); });
        enqueue_merge(c, p.n_slices * k, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
    }
    HIP_OK(hipGetLastError(), err, -3);
    return eng_->op_end(op, err) ? 0 : -3;
}

// out_ids_ / out_scores_ [nq][k], which a search or rescore (what) on stream() has filled -> host; the caller's arrays are written only on success
int TokenIndex::deliver_results(const char *what, int nq, int k, int32_t *ids, float *scores, std::string &err) {
    HostResults res((size_t)nq * k);
    if (!results_to_host(stream_, 0, res.ids.size(), res, err)) { err = std::string(what) + ": " + err; return -3; }
    res.deliver(ids, scores);
    return 0;
}

int TokenIndex::search_to_host(int nq, const int32_t *d_qcu, const void *d_q, bool q_f32, int max_q_len, int k, int32_t *ids, float *scores,
                               std::string &err, const uint32_t *d_allow) {
    if (!grow(out_ids_, (size_t)nq * k * 4, err) || !grow(out_scores_, (size_t)nq * k * 4, err)) return -3;
    if (const int r = search_any(nq, d_qcu, d_q, q_f32, max_q_len, k, out_ids_.as<int32_t>(), out_scores_.as<float>(), stream_, err, d_allow); r != 0) {
        (void)hipStreamSynchronize(stream_);
        return r;
    }
    return deliver_results("search", nq, k, ids, scores, err);
}

int TokenIndex::stage_queries(const char *what, int nq, const int32_t *qcu, const float *q_rows, int limit, int &max_len, std::string &err) {
    if (!token_cu_ok(qcu, nq)) { err = std::string(what) + ": qcu must ascend strictly from an entry >= 0 (no empty query)"; return -2; }
    max_len = 0;
    for (int i = 0; i < nq; ++i) max_len = std::max(max_len, qcu[i + 1] - qcu[i]);
    if (limit > 0 && max_len > limit) {
        err = std::string(what) + ": a query of " + std::to_string(max_len) + " tokens; a search at dim " + std::to_string(dim_) + " takes at most " + std::to_string(limit);
        return -2;
    }
    const size_t T = (size_t)(qcu[nq] - qcu[0]), n = T * dim_;
    if (n > F32_TO_F16_MAX_N) { err = std::string(what) + ": more than 2^31 query values (tokens x dim) in one call"; return -2; }
    if (!grow(stage_, n * 4, err) || (dtype_ != 2 && !grow(q16_, n * 2, err)) || !grow(qcu_in_, (size_t)(nq + 1) * 4, err)) return -3;
    // (the previous host call has synchronised stream(): nothing reads the staged lengths any more)
    qcu_h_.resize((size_t)nq + 1);
    for (int i = 0; i <= nq; ++i) qcu_h_[i] = qcu[i] - qcu[0];
    HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -3);
    HIP_OK(hipMemcpyAsync(stage_.p, q_rows + (size_t)qcu[0] * dim_, n * 4, hipMemcpyHostToDevice, stream_), err, -3);
    HIP_OK(hipMemcpyAsync(qcu_in_.p, qcu_h_.data(), qcu_h_.size() * 4, hipMemcpyHostToDevice, stream_), err, -3);
    // (the int8 form quantises the f32 rows where they are)
    if (dtype_ != 2) eng_->timed_launch("f32_to_f16", 0.0, stream_, [&] { launch_f32_to_f16(stage_.as<float>(), q16_.as<half_t>(), n, stream_); });
    HIP_OK(hipGetLastError(), err, -3);
    return 0;
}

int TokenIndex::search_host(int nq, const int32_t *qcu, const float *q_rows, int k, int32_t *ids, float *scores, std::string &err,
                            const uint32_t *allow) {
    if (const int go = check_search(nq, qcu, q_rows, k, ids, scores, err); go <= 0) return go;
    DeviceGuard g(eng_->device());
    int max_len = 0;
    if (const int r = stage_queries("search", nq, qcu, q_rows, max_query_tokens(), max_len, err); r != 0) { (void)hipStreamSynchronize(stream_); return r; }
    const uint32_t *d_allow = nullptr;
    if (!upload_allow(allow, stream_, d_allow, err)) { (void)hipStreamSynchronize(stream_); return -3; }
    return search_to_host(nq, qcu_in_.as<int32_t>(), dtype_ == 2 ? stage_.p : q16_.p, dtype_ == 2, max_len, k, ids, scores, err, d_allow);
}

// ------------------------------------------------------------------------------------------------
// rescoring
// ------------------------------------------------------------------------------------------------
int TokenIndex::rescore_device(int nq, const int32_t *d_qcu, const half_t *d_q, int n_cand, const int32_t *d_cand, int k, int32_t *d_ids,
                               float *d_scores, hipStream_t s, std::string &err) {
    if (const int go = check_rescore(nq, d_qcu, d_q, n_cand, d_cand, k, d_ids, d_scores, err); go <= 0) return go;
    if ((uintptr_t)d_q & 15) { err = "rescore: the query rows must be 16-byte aligned"; return -2; }
    // (the int8 form: the scan's kernel over the candidate lists; the device form knows no query length, so the launch is sized for the
    // longest a search takes)
    if (dtype_ == 2) return scan_chunks(nq, d_qcu, d_q, false, max_query_tokens(), k, d_ids, d_scores, s, err, nullptr, d_cand, n_cand);
    DeviceGuard g(eng_->device());
    Engine::StreamOp op;
    if (!eng_->op_begin(s, busy_, op, err)) return -3;
    const size_t ent = (size_t)std::min(nq, QCHUNK) * n_cand;
    if (!grow(ws_s_, ent * 4, err) || !grow(ws_i_, ent * 4, err) || !grow(pairs_, ent * 8, err)) return -3;
    for (int c0 = 0; c0 < nq; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, nq - c0);
        TokenPairsArgs pa{d_cand + (size_t)c0 * n_cand, pairs_.as<int32_t>(), ws_i_.as<int>(), c, n_cand, n_, live_};
        eng_->timed_launch("token_index_pairs", 0.0, s, [&] { launch_token_pairs(pa, s); });
        // (the index's own arrays are maxsim's document side; a pair (q, -1) is scored NaN and reads nothing)
        MaxsimArgs ma{d_q, (const half_t *)rows_, d_qcu + c0, cu_, pairs_.as<int32_t>(), ws_s_.as<float>(), c, n_, dim_, c * n_cand, 0, 0};
        eng_->timed_launch("maxsim", 0.0, s, [&] { launch_maxsim(ma, s, eng_->options().maxsim_launch_pairs); });
        enqueue_merge(c, n_cand, k, d_ids + (size_t)c0 * k, d_scores + (size_t)c0 * k, s);
    }
    HIP_OK(hipGetLastError(), err, -3);
    return eng_->op_end(op, err) ? 0 : -3;
}

int TokenIndex::rescore_host(int nq, const int32_t *qcu, const float *q_rows, int n_cand, const int32_t *cand, int k, int32_t *ids, float *scores,
                             std::string &err) {
    if (const int go = check_rescore(nq, qcu, q_rows, n_cand, cand, k, ids, scores, err); go <= 0) return go;
    for (size_t i = 0; i < (size_t)nq * n_cand; ++i)
        if (cand[i] < -1 || cand[i] >= n_) { err = "rescore: candidate id " + std::to_string(cand[i]) + " is outside [-1, " + std::to_string(n_) + ")"; return -2; }
    DeviceGuard g(eng_->device());
    if (!grow(cand_in_, (size_t)nq * n_cand * 4, err) || !grow(out_ids_, (size_t)nq * k * 4, err) || !grow(out_scores_, (size_t)nq * k * 4, err)) return -3;
    int max_len = 0;
    if (const int r = stage_queries("rescore", nq, qcu, q_rows, dtype_ == 2 ? max_query_tokens() : 0, max_len, err); r != 0) { (void)hipStreamSynchronize(stream_); return r; }
    auto fail = [&](int r) { (void)hipStreamSynchronize(stream_); return r; };
    if (hipMemcpyAsync(cand_in_.p, cand, (size_t)nq * n_cand * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) { err = "rescore: copy to the device failed"; return fail(-3); }
    if (const int r = dtype_ == 2 ? scan_chunks(nq, qcu_in_.as<int32_t>(), stage_.p, true, max_len, k, out_ids_.as<int32_t>(), out_scores_.as<float>(), stream_, err,
                                                nullptr, cand_in_.as<int32_t>(), n_cand)
                                  : rescore_device(nq, qcu_in_.as<int32_t>(), q16_.as<half_t>(), n_cand, cand_in_.as<int32_t>(), k, out_ids_.as<int32_t>(),
                                                   out_scores_.as<float>(), stream_, err); r != 0) return fail(r);
    return deliver_results("rescore", nq, k, ids, scores, err);
}

// ------------------------------------------------------------------------------------------------
// removed documents, compaction, file form
// ------------------------------------------------------------------------------------------------
int TokenIndex::remove(int n, const int32_t *ids, std::string &err) {
    std::vector<int32_t> fresh;                          // the ids this call removes (repeats and removed documents left out)
    const Removed r = remove_rows(n, ids, cap_docs_, fresh, err);
    if (r != Removed::ok) return r == Removed::refused ? -2 : -3;
    for (int32_t id : fresh) tok_removed_ += cu_h_[(size_t)id + 1] - cu_h_[(size_t)id];
    return (int)fresh.size();
}

int TokenIndex::compact(int32_t *old_ids, std::string &err) {
    if (dtype_ == 2) { err = "compact: not available for an int8 token index"; return -2; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -3);
    HIP_OK(hipStreamSynchronize(stream_), err, -3);
    if (bits_.n_removed == 0) return compact_nothing(old_ids);
    // the kept documents' former ids and their new cumulative lengths, from the mirrors
    const int nl = n_live();
    const int64_t ntl = n_live_tokens();
    const std::vector<int32_t> map = bits_.kept(n_);
    std::vector<int32_t> ncu((size_t)nl + 1, 0);
    for (int j = 0; j < nl; ++j) ncu[(size_t)j + 1] = ncu[(size_t)j] + (cu_h_[(size_t)map[(size_t)j] + 1] - cu_h_[(size_t)map[(size_t)j]]);
    // everything new is made before anything old is let go: fresh lengths and fresh rows beside the old ones (the peak is old + new)
    const int cap = std::max(nl, 1024);
    int32_t *pc = nullptr, *d_map = nullptr;
    half_t *pr = nullptr;
    const char *failed = nullptr;
    if (hipMalloc((void **)&pc, ((size_t)cap + 1) * 4) != hipSuccess || (nl > 0 && hipMalloc((void **)&d_map, (size_t)nl * 4) != hipSuccess) ||
        (ntl > 0 && hipMalloc((void **)&pr, (size_t)ntl * dim_ * 2) != hipSuccess)) failed = "hipMalloc (token index rows) failed";
    else if (hipMemcpyAsync(pc, ncu.data(), ncu.size() * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
             (nl > 0 && hipMemcpyAsync(d_map, map.data(), (size_t)nl * 4, hipMemcpyHostToDevice, stream_) != hipSuccess)) failed = "hipMemcpy (compaction ids) failed";
    else {
        if (nl > 0) {
            TokenGatherArgs a{(const half_t *)rows_, pr, cu_, pc, d_map, nl, dim_};
            eng_->timed_launch("token_index_gather", 0.0, stream_, [&] { launch_token_gather(a, stream_); });
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) failed = "the gather kernel failed";
    }
    if (d_map) (void)hipFree(d_map);
    if (failed) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream_);
        if (pc) (void)hipFree(pc);
        if (pr) (void)hipFree(pr);
        err = failed;
        return -3;
    }
    if (rows_) (void)hipFree(rows_);
    if (cu_) (void)hipFree(cu_);
    rows_ = (char *)pr; cu_ = pc;
    cap_tok_ = ntl; cap_docs_ = cap;
    n_ = nl; n_tok_ = ntl;
    cu_h_.swap(ncu);
    cu_h_.reserve((size_t)cap + 1);
    drop_live();
    tok_removed_ = 0;
    if (old_ids && nl > 0) memcpy(old_ids, map.data(), (size_t)nl * 4);
    return nl;
}

namespace {

// rows between HBM and a file in pieces of at most 32 MiB through a host buffer (index_io.h), as add uploads them: never a host copy of
// the index
constexpr size_t FILE_PIECE = (size_t)32 << 20;

}  // namespace

bool TokenIndex::save(const char *path, std::string &err) {
    if (!path || !*path) { err = "a path is required"; return false; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, false);
    HIP_OK(hipStreamSynchronize(stream_), err, false);
    TokenIndexFileHeader h;
    h.dim = (uint32_t)dim_; h.n_docs = (uint32_t)n_; h.has_live = live_ ? 1u : 0u; h.n_tokens = (uint64_t)n_tok_;
    unsigned char hdr[INDEX_HEADER_BYTES];
    token_index_header_write(h, hdr);
    return write_atomically(path, err, [&](FILE *f) {
        std::vector<char> buf;
        // (the lengths and the live words come from the mirrors; the mirror's bits at and beyond size are zero)
        return fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr && fwrite(cu_h_.data(), 4, (size_t)n_ + 1, f) == (size_t)n_ + 1 &&
               device_to_file(f, rows_, (size_t)n_tok_ * dim_ * 2, FILE_PIECE, buf, err) &&
               (!live_ || fwrite(bits_.words.data(), 4, live_words(n_), f) == live_words(n_));
    });
}

TokenIndex *TokenIndex::load(Engine *eng, FILE *f, const TokenIndexFileHeader &h, std::string &err) {
    const int n = (int)h.n_docs;
    // the lengths and the live words stand on both sides of the rows: read and checked first, in front of any allocation on the device
    std::vector<int32_t> cu((size_t)n + 1);
    if (fread(cu.data(), 4, cu.size(), f) != cu.size()) { err = "read failed"; return nullptr; }
    if (!token_index_cu_check(h, cu.data(), err)) return nullptr;
    std::vector<uint32_t> words(h.has_live ? live_words(n) : 0);
    const uint64_t rows_at = INDEX_HEADER_BYTES + token_index_file_cu_bytes(h), bytes = token_index_file_row_bytes(h);
    if (fseeko(f, (off_t)(rows_at + bytes), SEEK_SET) != 0 || fread(words.data(), 4, words.size(), f) != words.size()) { err = "read failed"; return nullptr; }
    if (!token_index_live_check(h, words.data(), err)) return nullptr;
    std::unique_ptr<TokenIndex> ix(create(eng, (int)h.dim, err));
    if (!ix) return nullptr;
    DeviceGuard g(eng->device());
    if (n == 0) {
        // (an empty index that had a bitmap keeps one: the file's bytes come back from a save)
        if (h.has_live && !ix->make_live(ix->cap_docs_, err)) return nullptr;
        return ix.release();
    }
    if (!ix->grow_storage(n, (long long)h.n_tokens, err)) return nullptr;
    if (fseeko(f, (off_t)rows_at, SEEK_SET) != 0) { err = "read failed"; return nullptr; }
    std::vector<char> buf;
    if (!file_to_device(f, ix->rows_, (size_t)bytes, FILE_PIECE, buf, err)) return nullptr;
    // (grow_storage reserved the mirror: its entries do not move afterwards)
    ix->cu_h_.assign(cu.begin(), cu.end());
    HIP_OK(hipMemcpy(ix->cu_, ix->cu_h_.data(), ix->cu_h_.size() * 4, hipMemcpyHostToDevice), err, nullptr);
    ix->n_ = n;
    ix->n_tok_ = (int64_t)h.n_tokens;
    if (!h.has_live) return ix.release();
    if (!ix->install_live(words.data(), ix->cap_docs_, err)) return nullptr;
    for (int d = 0; d < n; ++d)
        if (!ix->bits_.test(d)) ix->tok_removed_ += cu[(size_t)d + 1] - cu[(size_t)d];
    return ix.release();
}

bool TokenIndex::text_buffers(size_t in_bytes, size_t out_bytes, char *&d_in, char *&d_out, std::string &err) {
    if (!grow(text_in_, in_bytes, err) || !grow(text_out_, std::max<size_t>(out_bytes, 16), err)) return false;
    d_in = text_in_.as<char>();
    d_out = text_out_.as<char>();
    return true;
}

}  // namespace bert_hip
