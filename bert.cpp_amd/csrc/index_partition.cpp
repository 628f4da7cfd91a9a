// index_partition.cpp — the cluster partition of an embedding index (search.h): the assignment of rows to centroids, the list
// tables on the device (built by partition.h), k-means, and the partition file.  The probed search that reads the tables is in
// index.cpp.
//
// The assignment is a public search: the list of a row is the id that a k = 1 search of an f32 index of the centroids returns
// for the row as get_rows gives it; -1 (every score NaN) becomes list 0.  partition and kmeans share assign_rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include <sys/stat.h>

#include "index_io.h"
#include "partition.h"
#include "search.h"
#include "search_kernels.h"

namespace bert_hip {

// list_of [size]: every row's list among cent's rows, removed rows included.  Blocking, on the index's stream.
bool Index::assign_rows(Index &cent, std::vector<int32_t> &list_of, std::string &err) {
    list_of.assign((size_t)n_, 0);
    const int nqc = std::min(n_, QCHUNK);
    if (!grow(export_, (size_t)nqc * dim_ * 4, err) || !grow(assign_i_, (size_t)nqc * 4, err) || !grow(assign_s_, (size_t)nqc * 4, err)) return false;
    for (int c0 = 0; c0 < n_; c0 += QCHUNK) {
        const int c = std::min(QCHUNK, n_ - c0);
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, false);
        enqueue_export(c0, c, nullptr, export_.as<float>(), stream_);
        HIP_OK(hipGetLastError(), err, false);
        HIP_OK(hipEventRecord(busy_, stream_), err, false);
        if (cent.search_device(c, export_.as<float>(), 1, assign_i_.as<int32_t>(), assign_s_.as<float>(), stream_, err) != 0) {
            (void)hipStreamSynchronize(stream_);
            return false;
        }
        HIP_OK(hipMemcpyAsync(list_of.data() + c0, assign_i_.p, (size_t)c * 4, hipMemcpyDeviceToHost, stream_), err, false);
        HIP_OK(hipStreamSynchronize(stream_), err, false);
    }
    for (int32_t &l : list_of)
        if (l < 0) l = 0;
    return true;
}

namespace {

// the tables of list_of into two device buffers (which only grow); blocking
bool upload_tables(const std::vector<int32_t> &list_of, int n_lists, DevBuf &offsets, DevBuf &order, std::string &err) {
    ListTables t;
    build_lists(list_of.data(), (int)list_of.size(), n_lists, t);
    if (!offsets.ensure(t.offsets.size() * 4, err) || !order.ensure(std::max<size_t>(t.order.size(), 1) * 4, err)) return false;
    HIP_OK(hipMemcpy(offsets.p, t.offsets.data(), t.offsets.size() * 4, hipMemcpyHostToDevice), err, false);
    if (!t.order.empty()) HIP_OK(hipMemcpy(order.p, t.order.data(), t.order.size() * 4, hipMemcpyHostToDevice), err, false);
    return true;
}

}  // namespace

bool Index::upload_lists(const std::vector<int32_t> &list_of, int n_lists, std::string &err) {
    HIP_OK(hipEventSynchronize(busy_), err, false);          // (what is queued may still read the old tables)
    return upload_tables(list_of, n_lists, offsets_, order_, err);
}

void Index::drop_partition() {
    cent_.reset();
    cent_h_.clear();
    list_of_.clear();
    n_part_ = 0;
}

int Index::partition(int n_lists, const float *centroids, std::string &err) {
    if (n_lists < 0 || n_lists > MAX_LISTS || (n_lists > 0 && !centroids)) { err = "partition: 0 <= n_lists <= 65536 and centroids required"; return -1; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -1);
    if (n_lists == 0) { drop_partition(); return 0; }
    // (the index keeps its partition until the new one is complete)
    std::unique_ptr<Index> cent(Index::create(eng_, dim_, 0, err));
    if (!cent || cent->add_host(n_lists, centroids, err) < 0) return -1;
    std::vector<int32_t> list_of;
    if (!assign_rows(*cent, list_of, err)) return -1;
    return install_partition(std::move(cent), centroids, std::move(list_of), err) ? 0 : -1;
}

// cent (the centroids as an index), centroids (the same on the host) and the lists of the first list_of.size() rows become the
// partition; on an error the index keeps the one it had
bool Index::install_partition(std::unique_ptr<Index> cent, const float *centroids, std::vector<int32_t> &&list_of, std::string &err) {
    const int n_lists = cent->size();
    if (!upload_lists(list_of, n_lists, err)) {
        std::string e2;
        if (cent_ && !upload_lists(list_of_, this->n_lists(), e2)) drop_partition();    // (the tables of the partition that stays)
        return false;
    }
    cent_ = std::move(cent);
    cent_h_.assign(centroids, centroids + (size_t)n_lists * dim_);
    n_part_ = (int)list_of.size();
    list_of_ = std::move(list_of);
    return true;
}

// ------------------------------------------------------------------------------------------------
// the partition file (index_file.h)
// ------------------------------------------------------------------------------------------------
bool Index::save_partition(const char *path, std::string &err) {
    if (!path || !*path) { err = "a path is required"; return false; }
    if (!cent_) { err = "the index has no partition"; return false; }
    PartitionFileHeader h;
    h.dim = (uint32_t)dim_; h.n_lists = (uint32_t)n_lists(); h.n_part = (uint32_t)n_part_;
    unsigned char hdr[INDEX_HEADER_BYTES];
    partition_header_write(h, hdr);
    return write_atomically(path, err, [&](FILE *f) {
        return fwrite(hdr, 1, sizeof hdr, f) == sizeof hdr && fwrite(cent_h_.data(), 4, cent_h_.size(), f) == cent_h_.size() &&
               fwrite(list_of_.data(), 4, (size_t)n_part_, f) == (size_t)n_part_;
    });
}

int Index::load_partition(const char *path, std::string &err) {
    if (!path || !*path) { err = "a path is required"; return -2; }
    FILE *f = fopen(path, "rb");
    struct stat st;
    if (!f || fstat(fileno(f), &st) != 0 || !S_ISREG(st.st_mode)) {
        if (f) fclose(f);
        err = "cannot read '" + std::string(path) + "'";
        return -3;
    }
    // the header and the file's length first; then the contents, on the host; the device only sees a partition that passed
    unsigned char hdr[INDEX_HEADER_BYTES];
    const size_t got = fread(hdr, 1, sizeof hdr, f);
    PartitionFileHeader h;
    std::vector<float> cents;
    std::vector<int32_t> list_of;
    int r = 0;
    if (!partition_header_check(hdr, got, (uint64_t)st.st_size, h, err)) r = -2;
    else if ((int)h.dim != dim_) { err = "the file has dim " + std::to_string(h.dim) + ", the index " + std::to_string(dim_); r = -2; }
    else if (h.n_part > (uint32_t)n_) { err = "the file assigns " + std::to_string(h.n_part) + " rows, the index holds " + std::to_string(n_); r = -2; }
    else {
        cents.resize((size_t)h.n_lists * h.dim);
        list_of.resize(h.n_part);
        if (fread(cents.data(), 4, cents.size(), f) != cents.size() || fread(list_of.data(), 4, list_of.size(), f) != list_of.size()) { err = "read failed"; r = -3; }
    }
    fclose(f);
    if (r != 0) return r;
    for (float c : cents)
        if (!std::isfinite(c)) { err = "a centroid element is not finite"; return -2; }
    for (size_t i = 0; i < list_of.size(); ++i)
        if (list_of[i] < 0 || list_of[i] >= (int32_t)h.n_lists) {
            err = "row " + std::to_string(i) + " has list id " + std::to_string(list_of[i]) + ", outside [0, " + std::to_string(h.n_lists) + ")";
            return -2;
        }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -3);
    std::unique_ptr<Index> cent(Index::create(eng_, dim_, 0, err));
    if (!cent || cent->add_host((int)h.n_lists, cents.data(), err) < 0) return -3;
    return install_partition(std::move(cent), cents.data(), std::move(list_of), err) ? 0 : -3;
}

void Index::partition_lists(int32_t *list_of_row) const {
    std::copy(list_of_.begin(), list_of_.end(), list_of_row);
    std::fill(list_of_row + n_part_, list_of_row + n_, -1);
}

int Index::kmeans(int n_lists, int n_iter, float *centroids, std::string &err) {
    if (n_lists < 1 || n_lists > MAX_LISTS || n_iter < 1 || !centroids) { err = "kmeans: 1 <= n_lists <= 65536, n_iter >= 1 and centroids required"; return -1; }
    DeviceGuard g(eng_->device());
    HIP_OK(hipEventSynchronize(busy_), err, -1);
    std::unique_ptr<Index> cent(Index::create(eng_, dim_, 0, err));
    if (!cent) return -1;
    const size_t cbytes = (size_t)n_lists * dim_ * 4;
    DevBuf d_cent, offsets, order;
    if (!d_cent.upload(centroids, cbytes, err)) return -1;
    std::vector<int32_t> list_of;
    for (int it = 0; it < n_iter; ++it) {
        // the centroids of this iteration as an index; the assignment; the lists of the live rows
        cent->truncate(0);
        if (cent->add_device(n_lists, d_cent.as<float>(), stream_, err) < 0 || !assign_rows(*cent, list_of, err)) return -1;
        if (live_)
            for (int r = 0; r < n_; ++r)
                if (!bits_.test(r)) list_of[(size_t)r] = -1;
        if (!upload_tables(list_of, n_lists, offsets, order, err)) return -1;
        KmeansArgs a;
        a.rows = rows_; a.rscale = rscale_; a.offsets = offsets.as<int32_t>(); a.order = order.as<int32_t>();
        a.centroids = d_cent.as<float>(); a.n_lists = n_lists; a.dim = dim_; a.dpad = dpad_;
        HIP_OK(hipStreamWaitEvent(stream_, busy_, 0), err, -1);
        eng_->timed_launch("kmeans_update", 0.0, stream_, [&] { launch_kmeans_update(dtype_, a, stream_); });
        HIP_OK(hipGetLastError(), err, -1);
        HIP_OK(hipEventRecord(busy_, stream_), err, -1);
        HIP_OK(hipStreamSynchronize(stream_), err, -1);
    }
    HIP_OK(hipMemcpy(centroids, d_cent.p, cbytes, hipMemcpyDeviceToHost), err, -1);
    return 0;
}

}  // namespace bert_hip
