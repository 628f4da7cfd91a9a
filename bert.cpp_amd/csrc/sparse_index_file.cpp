// sparse_index_file.cpp — header and body checks of a sparse index file (sparse_index_file.h).  No device, no alignment assumed.
#include "sparse_index_file.h"

#include <cstring>

#include "live_bits.h"

namespace bert_hip {

namespace {

const char SPARSE_MAGIC[8] = {'B', 'H', 'I', 'P', 'S', 'P', 'X', '1'};

void put_u32(unsigned char *p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (8 * i));
}

uint32_t get_u32(const unsigned char *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

uint64_t blocks_of(uint64_t rows) { return (rows + SPARSE_FILE_BLOCK_ROWS - 1) / SPARSE_FILE_BLOCK_ROWS; }

}  // namespace

uint64_t sparse_index_file_array_bytes(const SparseIndexFileHeader &h) {
    return blocks_of(h.n_rows) * (uint64_t)h.width * SPARSE_FILE_BLOCK_ROWS * sparse_file_elem_bytes(h.dtype);
}

uint64_t sparse_index_file_bytes(const SparseIndexFileHeader &h) {
    uint64_t n = INDEX_HEADER_BYTES + 2 * sparse_index_file_array_bytes(h) + (uint64_t)h.n_rows * 4;
    if (h.has_live) n += ((uint64_t)h.n_rows + 31) / 32 * 4;
    return n;
}

void sparse_index_header_write(const SparseIndexFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]) {
    memset(out, 0, INDEX_HEADER_BYTES);
    memcpy(out, SPARSE_MAGIC, 8);
    const uint32_t f[6] = {h.version, h.dtype, h.n_vocab, h.width, h.n_rows, h.has_live};
    for (int i = 0; i < 6; ++i) put_u32(out + 8 + 4 * i, f[i]);
}

bool sparse_index_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, SparseIndexFileHeader &h, std::string &err) {
    const unsigned char *p = (const unsigned char *)buf;
    if (!p || buf_len < INDEX_HEADER_BYTES) { err = "shorter than the 64-byte header"; return false; }
    if (memcmp(p, SPARSE_MAGIC, 8) != 0) { err = "not a sparse index file (magic BHIPSPX1 expected)"; return false; }
    SparseIndexFileHeader g;
    g.version = get_u32(p + 8); g.dtype = get_u32(p + 12); g.n_vocab = get_u32(p + 16);
    g.width = get_u32(p + 20); g.n_rows = get_u32(p + 24); g.has_live = get_u32(p + 28);
    if (g.version != SPARSE_INDEX_FILE_VERSION) { err = "version " + std::to_string(g.version) + " (this build reads version 1)"; return false; }
    if (g.dtype > 1) { err = "dtype " + std::to_string(g.dtype) + " (0 i32 + f32, 1 u16 + f16)"; return false; }
    if (g.n_vocab < 1 || g.n_vocab > SPARSE_FILE_MAX_VOCAB) { err = "n_vocab " + std::to_string(g.n_vocab) + " (1 .. 262144)"; return false; }
    if (g.dtype == 1 && g.n_vocab > 65536) { err = "n_vocab " + std::to_string(g.n_vocab) + " with dtype 1, whose u16 ids end at 65536"; return false; }
    if (g.width < 1 || g.width > SPARSE_FILE_MAX_WIDTH) { err = "width " + std::to_string(g.width) + " (1 .. 256)"; return false; }
    if (g.n_rows > 0x7fffffffu - SPARSE_FILE_BLOCK_ROWS) { err = "more than 2^31 - 65 rows"; return false; }
    if (g.has_live > 1) { err = "has_live " + std::to_string(g.has_live) + " (0 or 1)"; return false; }
    for (size_t i = 32; i < INDEX_HEADER_BYTES; ++i)
        if (p[i]) { err = "non-zero reserved header bytes"; return false; }
    const uint64_t want = sparse_index_file_bytes(g);
    if (file_bytes != want) {
        err = "the file has " + std::to_string(file_bytes) + " bytes, its header describes " + std::to_string(want) +
              (file_bytes < want ? " (truncated)" : " (over-long)");
        return false;
    }
    h = g;
    return true;
}

bool sparse_index_counts_check(const SparseIndexFileHeader &h, const int32_t *counts, std::string &err) {
    const unsigned char *p = (const unsigned char *)counts;
    for (uint64_t r = 0; r < h.n_rows; ++r) {
        const uint32_t c = get_u32(p + 4 * r);
        if (c > h.width) { err = "row " + std::to_string(r) + " has count " + std::to_string((int32_t)c) + " (0 .. " + std::to_string(h.width) + ")"; return false; }
    }
    return true;
}

bool sparse_index_ids_check(const SparseIndexFileHeader &h, const void *ids, uint64_t first_block, uint64_t n_blocks, const int32_t *counts,
                            std::string &err) {
    const unsigned char *p = (const unsigned char *)ids, *pc = (const unsigned char *)counts;
    const uint64_t eb = sparse_file_elem_bytes(h.dtype);
    for (uint64_t b = 0; b < n_blocks; ++b)
        for (uint64_t lane = 0; lane < SPARSE_FILE_BLOCK_ROWS; ++lane) {
            const uint64_t row = (first_block + b) * SPARSE_FILE_BLOCK_ROWS + lane;
            if (row >= h.n_rows) break;
            const uint32_t n = get_u32(pc + 4 * row);
            for (uint64_t j = 0; j < n; ++j) {
                const unsigned char *e = p + ((b * h.width + j) * SPARSE_FILE_BLOCK_ROWS + lane) * eb;
                const uint32_t id = eb == 2 ? (uint32_t)e[0] | (uint32_t)e[1] << 8 : get_u32(e);
                if (id >= h.n_vocab) {
                    err = "row " + std::to_string(row) + " column " + std::to_string(j) + " holds id " + std::to_string(eb == 2 ? (int64_t)id : (int64_t)(int32_t)id) +
                          " outside [0, " + std::to_string(h.n_vocab) + ")";
                    return false;
                }
            }
        }
    return true;
}

bool sparse_index_live_check(const SparseIndexFileHeader &h, const uint32_t *words, std::string &err) {
    if (!h.has_live || (h.n_rows & 31) == 0) return true;
    const uint32_t last = get_u32((const unsigned char *)words + 4 * (uint64_t)(h.n_rows >> 5));
    if (!live_tail_clear(last, h.n_rows)) { err = "live bits beyond the last row"; return false; }
    return true;
}

bool sparse_index_body_check(const SparseIndexFileHeader &h, const void *body, uint64_t body_len, std::string &err) {
    if (!body || body_len != sparse_index_file_bytes(h) - INDEX_HEADER_BYTES) { err = "the body's length is not what the header describes"; return false; }
    const unsigned char *p = (const unsigned char *)body;
    const uint64_t arr = sparse_index_file_array_bytes(h);
    const int32_t *counts = (const int32_t *)(p + 2 * arr);
    return sparse_index_counts_check(h, counts, err) && sparse_index_ids_check(h, p, 0, blocks_of(h.n_rows), counts, err) &&
           sparse_index_live_check(h, (const uint32_t *)(p + 2 * arr + (uint64_t)h.n_rows * 4), err);
}

}  // namespace bert_hip
