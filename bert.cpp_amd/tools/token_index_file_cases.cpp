// token_index_file_cases — token_index_file.cpp's header and body checks on their own, for a sanitizer build on the CPU: the cases of
// tests/test_late_index_host.py, each fed from a heap buffer of exactly its length, so that a read past the buffer, a shift or an
// overflow in the length arithmetic is caught.
//   make -C bert.cpp_amd check-host
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "token_index_file.h"

using namespace bert_hip;

namespace {

std::vector<unsigned char> header(uint32_t dim, uint32_t n_docs, uint32_t has_live, uint64_t n_tokens, uint32_t version = 1,
                                  const char *magic = "BHIPTOK1") {
    std::vector<unsigned char> h(INDEX_HEADER_BYTES, 0);
    memcpy(h.data(), magic, 8);
    const uint32_t f[6] = {version, dim, n_docs, has_live, (uint32_t)n_tokens, (uint32_t)(n_tokens >> 32)};
    for (int i = 0; i < 6; ++i)
        for (int b = 0; b < 4; ++b) h[8 + 4 * i + b] = (unsigned char)(f[i] >> (8 * b));
    return h;
}

uint64_t bytes_of(uint64_t dim, uint64_t n_docs, uint64_t has_live, uint64_t n_tokens) {
    return 64 + (n_docs + 1) * 4 + n_tokens * dim * 2 + (has_live ? (n_docs + 31) / 32 * 4 : 0);
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
    TokenIndexFileHeader h;
    std::string err;
    report(name, token_index_header_check(buf.empty() ? nullptr : p.get(), buf.size(), file_bytes, h, err), want, err);
}

// a body of n documents: document d has 1 + d % 3 tokens, rows zero, every document live
struct Body {
    TokenIndexFileHeader h;
    std::vector<unsigned char> b;
    Body(uint32_t dim, uint32_t n_docs, uint32_t has_live) {
        h.dim = dim; h.n_docs = n_docs; h.has_live = has_live;
        for (uint32_t d = 0; d < n_docs; ++d) h.n_tokens += 1 + d % 3;
        b.assign((size_t)(token_index_file_bytes(h) - INDEX_HEADER_BYTES), 0);
        uint32_t t = 0;
        for (uint32_t d = 0; d < n_docs; ++d) {
            t += 1 + d % 3;
            set_cu(d + 1, t);
            if (has_live) b[live_at() + d / 8] |= (unsigned char)(1u << (d % 8));
        }
    }
    size_t live_at() const { return (size_t)(token_index_file_cu_bytes(h) + token_index_file_row_bytes(h)); }
    void set_cu(uint32_t i, uint32_t v) { for (int k = 0; k < 4; ++k) b[(size_t)i * 4 + k] = (unsigned char)(v >> (8 * k)); }
    uint32_t cu(uint32_t i) const { return (uint32_t)b[(size_t)i * 4] | (uint32_t)b[(size_t)i * 4 + 1] << 8 | (uint32_t)b[(size_t)i * 4 + 2] << 16 | (uint32_t)b[(size_t)i * 4 + 3] << 24; }
    void expect(const char *name, bool want, size_t len = SIZE_MAX) const {
        if (len == SIZE_MAX) len = b.size();
        std::unique_ptr<unsigned char[]> p(new unsigned char[len ? len : 1]);
        if (!b.empty()) memcpy(p.get(), b.data(), std::min(len, b.size()));
        std::string err;
        report(name, token_index_body_check(h, p.get(), len, err), want, err);
    }
};

}  // namespace

int main() {
    const uint64_t good = bytes_of(384, 1000, 1, 25000);
    expect("good", header(384, 1000, 1, 25000), good, true);
    expect("good, no live words", header(64, 33, 0, 40), bytes_of(64, 33, 0, 40), true);
    expect("good, empty", header(8, 0, 0, 0), 68, true);
    expect("good, empty with live words", header(8, 0, 1, 0), 68, true);
    expect("good, largest (42 bits of length)", header(1024, 0x7fffffffu, 1, 0x7fffffffull), bytes_of(1024, 0x7fffffffu, 1, 0x7fffffffull), true);
    expect("good, past 2^41 bytes", header(1024, 1000, 0, 1100000000ull), bytes_of(1024, 1000, 0, 1100000000ull), true);
    expect("written by token_index_header_write", [] {
        TokenIndexFileHeader h;
        h.dim = 1024; h.n_docs = 65; h.has_live = 1; h.n_tokens = 0x7ffffffeull;
        std::vector<unsigned char> b(INDEX_HEADER_BYTES);
        token_index_header_write(h, b.data());
        return b;
    }(), bytes_of(1024, 65, 1, 0x7ffffffeull), true);
    expect("wrong magic", header(384, 1000, 1, 25000, 1, "BHIPSPX1"), good, false);
    expect("version 2", header(384, 1000, 1, 25000, 2), good, false);
    expect("dim 0", header(0, 1000, 1, 25000), bytes_of(0, 1000, 1, 25000), false);
    expect("dim 12", header(12, 1000, 1, 25000), bytes_of(12, 1000, 1, 25000), false);
    expect("dim 1032", header(1032, 1000, 1, 25000), bytes_of(1032, 1000, 1, 25000), false);
    expect("n_tokens 2^31", header(8, 1000, 0, 0x80000000ull), bytes_of(8, 1000, 0, 0x80000000ull), false);
    expect("n_tokens 2^32 + 25000", header(384, 1000, 1, 0x100000000ull + 25000), good, false);
    expect("n_docs > n_tokens", header(8, 41, 0, 40), bytes_of(8, 41, 0, 40), false);
    expect("has_live 2", header(384, 1000, 2, 25000), good, false);
    {
        std::vector<unsigned char> b = header(384, 1000, 1, 25000);
        b[63] = 1;
        expect("non-zero last reserved byte", b, good, false);
        b[63] = 0; b[32] = 1;
        expect("non-zero first reserved byte", b, good, false);
    }
    {
        std::vector<unsigned char> b = header(384, 1000, 1, 25000);
        b.resize(63);
        expect("short buffer", b, good, false);
        expect("empty buffer", {}, good, false);
        b.resize(1);
        expect("one byte", b, 1, false);
    }
    expect("file one byte short", header(384, 1000, 1, 25000), good - 1, false);
    expect("file one byte long", header(384, 1000, 1, 25000), good + 1, false);
    expect("header only", header(384, 1000, 1, 25000), 64, false);
    expect("length equal modulo 2^32", header(1024, 1000, 0, 1100000000ull), bytes_of(1024, 1000, 0, 1100000000ull) & 0xffffffffu, false);

    Body(8, 0, 0).expect("body: empty", true);
    Body(8, 0, 1).expect("body: empty with live words", true);
    Body(8, 1, 1).expect("body: one document", true);
    Body(64, 300, 1).expect("body: 300 documents", true);
    Body(8, 65, 0).expect("body: one byte short", false, Body(8, 65, 0).b.size() - 1);
    { Body b(8, 65, 1); b.set_cu(0, 1); b.expect("body: cu[0] = 1", false); }
    { Body b(8, 65, 1); b.set_cu(0, 0xffffffffu); b.expect("body: cu[0] = -1", false); }
    { Body b(8, 65, 1); b.set_cu(7, b.cu(6)); b.expect("body: an equal pair (an empty document)", false); }
    { Body b(8, 65, 1); b.set_cu(7, b.cu(6) - 1); b.expect("body: a descent", false); }
    { Body b(8, 65, 1); b.set_cu(7, 0x80000005u); b.expect("body: a negative entry", false); }
    { Body b(8, 65, 1); b.set_cu(64, b.cu(65)); b.set_cu(65, b.cu(65) + 1); b.expect("body: the last entry beyond n_tokens", false); }
    { Body b(8, 65, 1); b.set_cu(65, b.cu(65) - 1); b.expect("body: the last entry below n_tokens", false); }
    { Body b(8, 65, 1); b.b.back() |= 0x80; b.expect("body: a live bit beyond n_docs", false); }
    { Body b(8, 65, 1); b.b[b.live_at() + 8] |= 0x02; b.expect("body: a live bit at n_docs", false); }
    { Body b(8, 64, 1); b.b.back() = 0x7f; b.expect("body: a removed last document of a full word", true); }
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
