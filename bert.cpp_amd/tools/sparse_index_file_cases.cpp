// sparse_index_file_cases — sparse_index_file.cpp's header and body checks on their own, for a sanitizer build on the CPU: the cases
// of tests/test_sparse_index_file_host.py, each fed from a heap buffer of exactly its length, so that a read past the buffer, a shift
// or an overflow in the length arithmetic is caught.
//   make -C bert.cpp_amd check-host
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sparse_index_file.h"

using namespace bert_hip;

namespace {

std::vector<unsigned char> header(uint32_t dtype, uint32_t n_vocab, uint32_t width, uint32_t n_rows, uint32_t has_live, uint32_t version = 1,
                                  const char *magic = "BHIPSPX1") {
    std::vector<unsigned char> h(INDEX_HEADER_BYTES, 0);
    memcpy(h.data(), magic, 8);
    const uint32_t f[6] = {version, dtype, n_vocab, width, n_rows, has_live};
    for (int i = 0; i < 6; ++i)
        for (int b = 0; b < 4; ++b) h[8 + 4 * i + b] = (unsigned char)(f[i] >> (8 * b));
    return h;
}

uint64_t bytes_of(uint64_t dtype, uint64_t width, uint64_t n_rows, uint64_t has_live) {
    return 64 + 2 * ((n_rows + 63) / 64 * width * 64 * (dtype == 1 ? 2 : 4)) + n_rows * 4 + (has_live ? (n_rows + 31) / 32 * 4 : 0);
}

int failures = 0;

void report(const char *name, bool got, bool want, const std::string &err) {
    const bool ok = got == want && (got || !err.empty());
    printf("%-4s %-52s %s\n", ok ? "ok" : "FAIL", name, got ? "accepted" : err.c_str());
    failures += !ok;
}

void expect(const char *name, const std::vector<unsigned char> &buf, uint64_t file_bytes, bool want) {
    // (a heap copy of exactly buf.size() bytes: the sanitizer sees a read beyond it)
    std::unique_ptr<unsigned char[]> p(new unsigned char[buf.size() ? buf.size() : 1]);
    if (!buf.empty()) memcpy(p.get(), buf.data(), buf.size());
    SparseIndexFileHeader h;
    std::string err;
    report(name, sparse_index_header_check(buf.empty() ? nullptr : p.get(), buf.size(), file_bytes, h, err), want, err);
}

// a body of n rows: row r has min(r % (width + 1), width) terms with ids j (ascending), weights zero, every row live
struct Body {
    SparseIndexFileHeader h;
    std::vector<unsigned char> b;
    size_t arr, eb;
    Body(uint32_t dtype, uint32_t n_vocab, uint32_t width, uint32_t n_rows, uint32_t has_live) {
        h.dtype = dtype; h.n_vocab = n_vocab; h.width = width; h.n_rows = n_rows; h.has_live = has_live;
        eb = dtype == 1 ? 2 : 4;
        arr = (size_t)sparse_index_file_array_bytes(h);
        b.assign((size_t)(sparse_index_file_bytes(h) - INDEX_HEADER_BYTES), 0);
        for (uint32_t r = 0; r < n_rows; ++r) {
            const uint32_t n = r % (width + 1);
            set_count(r, n);
            for (uint32_t j = 0; j < n; ++j) set_id(r, j, j % n_vocab);
            if (has_live) b[2 * arr + (size_t)n_rows * 4 + r / 8] |= (unsigned char)(1u << (r % 8));
        }
    }
    void set_count(uint32_t r, uint32_t n) { for (int i = 0; i < 4; ++i) b[2 * arr + (size_t)r * 4 + i] = (unsigned char)(n >> (8 * i)); }
    void set_id(uint32_t r, uint32_t j, uint32_t id) {
        const size_t o = (((size_t)(r / 64) * h.width + j) * 64 + r % 64) * eb;
        for (size_t i = 0; i < eb; ++i) b[o + i] = (unsigned char)(id >> (8 * i));
    }
    void expect(const char *name, bool want, size_t len = SIZE_MAX) const {
        if (len == SIZE_MAX) len = b.size();
        std::unique_ptr<unsigned char[]> p(new unsigned char[len ? len : 1]);
        if (!b.empty()) memcpy(p.get(), b.data(), std::min(len, b.size()));
        std::string err;
        report(name, sparse_index_body_check(h, p.get(), len, err), want, err);
    }
};

}  // namespace

int main() {
    const uint64_t good = bytes_of(0, 128, 1000, 1);
    expect("good", header(0, 30522, 128, 1000, 1), good, true);
    expect("good, f16", header(1, 30522, 128, 1000, 0), bytes_of(1, 128, 1000, 0), true);
    expect("good, empty", header(0, 1, 1, 0, 0), 64, true);
    expect("good, largest (41 bits of length)", header(0, 262144, 256, 0x7fffffffu - 64, 1), bytes_of(0, 256, 0x7fffffffu - 64, 1), true);
    expect("written by sparse_index_header_write", [] {
        SparseIndexFileHeader h;
        h.dtype = 1; h.n_vocab = 65536; h.width = 7; h.n_rows = 65; h.has_live = 1;
        std::vector<unsigned char> b(INDEX_HEADER_BYTES);
        sparse_index_header_write(h, b.data());
        return b;
    }(), bytes_of(1, 7, 65, 1), true);
    expect("wrong magic", header(0, 30522, 128, 1000, 1, 1, "BHIPIDX1"), good, false);
    expect("version 2", header(0, 30522, 128, 1000, 1, 2), good, false);
    expect("dtype 2", header(2, 30522, 128, 1000, 1), good, false);
    expect("width 0", header(0, 30522, 0, 1000, 1), bytes_of(0, 0, 1000, 1), false);
    expect("width 257", header(0, 30522, 257, 1000, 1), bytes_of(0, 257, 1000, 1), false);
    expect("n_vocab 0", header(0, 0, 128, 1000, 1), good, false);
    expect("n_vocab 262145", header(0, 262145, 128, 1000, 1), good, false);
    expect("dtype 1 with n_vocab 65537", header(1, 65537, 128, 1000, 1), bytes_of(1, 128, 1000, 1), false);
    expect("has_live 2", header(0, 30522, 128, 1000, 2), good, false);
    expect("n_rows 2^31 - 64", header(0, 30522, 1, 0x7fffffffu - 63, 0), bytes_of(0, 1, 0x7fffffffu - 63, 0), false);
    {
        std::vector<unsigned char> b = header(0, 30522, 128, 1000, 1);
        b[63] = 1;
        expect("non-zero last reserved byte", b, good, false);
        b[63] = 0; b[32] = 1;
        expect("non-zero first reserved byte", b, good, false);
    }
    {
        std::vector<unsigned char> b = header(0, 30522, 128, 1000, 1);
        b.resize(63);
        expect("short buffer", b, good, false);
        expect("empty buffer", {}, good, false);
        b.resize(1);
        expect("one byte", b, 1, false);
    }
    expect("file one byte short", header(0, 30522, 128, 1000, 1), good - 1, false);
    expect("file one byte long", header(0, 30522, 128, 1000, 1), good + 1, false);
    expect("header only", header(0, 30522, 128, 1000, 1), 64, false);
    expect("length equal modulo 2^32", header(0, 262144, 256, 0x7fffffffu - 64, 1), bytes_of(0, 256, 0x7fffffffu - 64, 1) & 0xffffffffu, false);

    for (uint32_t dtype = 0; dtype < 2; ++dtype) {
        Body(dtype, 64, 4, 0, 0).expect("body: empty", true);
        Body(dtype, 64, 4, 1, 1).expect("body: one row", true);
        Body(dtype, 300, 256, 300, 1).expect("body: 300 rows of up to 256 terms", true);
        Body(dtype, 64, 4, 65, 0).expect("body: one byte short", false, Body(dtype, 64, 4, 65, 0).b.size() - 1);
        { Body b(dtype, 64, 4, 65, 1); b.set_count(64, 5); b.expect("body: a count of width + 1", false); }
        { Body b(dtype, 64, 4, 65, 1); b.set_count(3, 0xffffffffu); b.expect("body: a count of -1", false); }
        { Body b(dtype, 64, 4, 65, 1); b.set_id(64, 3, 64); b.expect("body: a used id = n_vocab", false); }
        { Body b(dtype, 64, 4, 65, 1); b.set_id(64, 3, 63); b.expect("body: a used id = n_vocab - 1", true); }
        { Body b(dtype, 64, 4, 65, 1); b.set_id(5, 3, 0xffffu); b.expect("body: an unused id out of range", true); }     // (row 5 has 0 terms)
        { Body b(dtype, 64, 4, 65, 1); b.b.back() |= 0x80; b.expect("body: a live bit beyond n_rows", false); }
        { Body b(dtype, 64, 4, 64, 1); b.b.back() = 0x7f; b.expect("body: a removed last row of a full word", true); }
    }
    { Body b(0, 64, 4, 65, 1); b.set_id(64, 3, 0x80000000u); b.expect("body: a negative i32 id", false); }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
