// partition_header_cases — index_file.cpp's partition_header_check on its own, for a sanitizer build on the CPU: the cases of
// tests/test_partition_file_host.py, each fed from a heap buffer of exactly its length, so that a read past the buffer, a
// shift or an overflow in the length arithmetic is caught.
//   make -C bert.cpp_amd check-host
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "index_file.h"

using namespace bert_hip;

namespace {

std::vector<unsigned char> header(uint32_t dim, uint32_t n_lists, uint32_t n_part, uint32_t version = 1, const char *magic = "BHIPPRT1") {
    std::vector<unsigned char> h(INDEX_HEADER_BYTES, 0);
    memcpy(h.data(), magic, 8);
    const uint32_t f[4] = {version, dim, n_lists, n_part};
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < 4; ++b) h[8 + 4 * i + b] = (unsigned char)(f[i] >> (8 * b));
    return h;
}

uint64_t bytes_of(uint64_t dim, uint64_t n_lists, uint64_t n_part) { return 64 + n_lists * dim * 4 + n_part * 4; }

int failures = 0;

void expect(const char *name, const std::vector<unsigned char> &buf, uint64_t file_bytes, bool want) {
    // (a heap copy of exactly buf.size() bytes: the sanitizer sees a read beyond it)
    std::unique_ptr<unsigned char[]> p(new unsigned char[buf.size() ? buf.size() : 1]);
    if (!buf.empty()) memcpy(p.get(), buf.data(), buf.size());
    PartitionFileHeader h;
    std::string err;
    const bool got = partition_header_check(buf.empty() ? nullptr : p.get(), buf.size(), file_bytes, h, err);
    const bool ok = got == want && (got || !err.empty());
    printf("%-4s %-52s %s\n", ok ? "ok" : "FAIL", name, got ? "accepted" : err.c_str());
    failures += !ok;
}

}  // namespace

int main() {
    const uint64_t good = bytes_of(384, 1024, 100000);
    expect("good", header(384, 1024, 100000), good, true);
    expect("good, smallest", header(1, 1, 0), bytes_of(1, 1, 0), true);
    expect("good, largest (34 bits of length)", header(2048, 65536, 0x7fffffffu), bytes_of(2048, 65536, 0x7fffffffu), true);
    expect("written by partition_header_write", [] {
        PartitionFileHeader h;
        h.dim = 72; h.n_lists = 12; h.n_part = 1500;
        std::vector<unsigned char> b(INDEX_HEADER_BYTES);
        partition_header_write(h, b.data());
        return b;
    }(), bytes_of(72, 12, 1500), true);
    expect("wrong magic", header(384, 1024, 100000, 1, "BHIPIDX1"), good, false);
    expect("version 2", header(384, 1024, 100000, 2), good, false);
    expect("dim 0", header(0, 1024, 100000), bytes_of(0, 1024, 100000), false);
    expect("dim 2049", header(2049, 1024, 100000), bytes_of(2049, 1024, 100000), false);
    expect("n_lists 0", header(384, 0, 100000), bytes_of(384, 0, 100000), false);
    expect("n_lists 65537", header(384, 65537, 100000), bytes_of(384, 65537, 100000), false);
    expect("n_part 2^31", header(384, 1024, 0x80000000u), bytes_of(384, 1024, 0x80000000u), false);
    {
        std::vector<unsigned char> b = header(384, 1024, 100000);
        b[63] = 1;
        expect("non-zero last reserved byte", b, good, false);
        b[63] = 0; b[24] = 1;
        expect("non-zero first reserved byte", b, good, false);
    }
    {
        std::vector<unsigned char> b = header(384, 1024, 100000);
        b.resize(63);
        expect("short buffer", b, good, false);
        expect("empty buffer", {}, good, false);
    }
    expect("file one byte short", header(384, 1024, 100000), good - 1, false);
    expect("file one byte long", header(384, 1024, 100000), good + 1, false);
    expect("header only", header(384, 1024, 100000), 64, false);
    expect("length equal modulo 2^32", header(2048, 65536, 0x7fffffffu), bytes_of(2048, 65536, 0x7fffffffu) & 0xffffffffu, false);
    expect("n_part bytes wrap to 0 modulo 2^32", header(384, 1024, 0x40000000u), bytes_of(384, 1024, 0), false);
    printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
