// index_file.cpp — headers of an embedding index file and of a partition file (index_file.h): layout, and the check in front of a load.
#include "index_file.h"

#include <cstring>

namespace bert_hip {

namespace {

const char MAGIC[8] = {'B', 'H', 'I', 'P', 'I', 'D', 'X', '1'};
const char PARTITION_MAGIC[8] = {'B', 'H', 'I', 'P', 'P', 'R', 'T', '1'};

void put_u32(unsigned char *p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (8 * i));
}

uint32_t get_u32(const unsigned char *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

}  // namespace

int index_elem_size(int dtype) { return dtype == 0 ? 4 : dtype == 1 ? 2 : dtype == 2 ? 1 : 0; }

int index_dpad(int dtype, int dim) {
    const int step = dtype == 3 ? 128 : dtype == 2 ? 32 : dtype == 1 ? 16 : 8;
    return (dim + step - 1) / step * step;
}

uint64_t index_row_bytes(int dtype, int dpad) {
    return dtype == 3 ? (uint64_t)dpad / 8 : (uint64_t)dpad * (uint64_t)index_elem_size(dtype);
}

uint64_t index_file_bytes(const IndexFileHeader &h) {
    uint64_t n = INDEX_HEADER_BYTES + (uint64_t)h.n_rows * index_row_bytes((int)h.dtype, (int)h.dpad);
    if (h.dtype == 2) n += (uint64_t)h.n_rows * 4;
    if (h.has_live) n += ((uint64_t)h.n_rows + 31) / 32 * 4;
    return n;
}

void index_header_write(const IndexFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]) {
    memset(out, 0, INDEX_HEADER_BYTES);
    memcpy(out, MAGIC, 8);
    const uint32_t f[6] = {h.version, h.dtype, h.dim, h.dpad, h.n_rows, h.has_live};
    for (int i = 0; i < 6; ++i) put_u32(out + 8 + 4 * i, f[i]);
}

bool index_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, IndexFileHeader &h, std::string &err) {
    const unsigned char *p = (const unsigned char *)buf;
    if (!p || buf_len < INDEX_HEADER_BYTES) { err = "shorter than the 64-byte header"; return false; }
    if (memcmp(p, MAGIC, 8) != 0) { err = "not an index file (magic BHIPIDX1 expected)"; return false; }
    IndexFileHeader g;
    g.version = get_u32(p + 8); g.dtype = get_u32(p + 12); g.dim = get_u32(p + 16);
    g.dpad = get_u32(p + 20); g.n_rows = get_u32(p + 24); g.has_live = get_u32(p + 28);
    if (g.version != INDEX_FILE_VERSION) { err = "version " + std::to_string(g.version) + " (this build reads version 1)"; return false; }
    if (g.dtype > 3) { err = "dtype " + std::to_string(g.dtype) + " (0 f32, 1 f16, 2 i8, 3 b1)"; return false; }
    if (g.dim < 1 || g.dim > (uint32_t)INDEX_MAX_DIM) { err = "dim " + std::to_string(g.dim) + " (1 .. 2048)"; return false; }
    const uint32_t dpad = (uint32_t)index_dpad((int)g.dtype, (int)g.dim);
    if (g.dpad != dpad) { err = "dpad " + std::to_string(g.dpad) + " where dim " + std::to_string(g.dim) + " is stored in " + std::to_string(dpad); return false; }
    if (g.n_rows > 0x7fffffffu) { err = "more than 2^31 - 1 rows"; return false; }
    if (g.has_live > 1) { err = "has_live " + std::to_string(g.has_live) + " (0 or 1)"; return false; }
    for (size_t i = 32; i < INDEX_HEADER_BYTES; ++i)
        if (p[i]) { err = "non-zero reserved header bytes"; return false; }
    const uint64_t want = index_file_bytes(g);
    if (file_bytes != want) {
        err = "the file has " + std::to_string(file_bytes) + " bytes, its header describes " + std::to_string(want) +
              (file_bytes < want ? " (truncated)" : " (over-long)");
        return false;
    }
    h = g;
    return true;
}

uint64_t partition_file_bytes(const PartitionFileHeader &h) {
    return INDEX_HEADER_BYTES + (uint64_t)h.n_lists * (uint64_t)h.dim * 4 + (uint64_t)h.n_part * 4;
}

void partition_header_write(const PartitionFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]) {
    memset(out, 0, INDEX_HEADER_BYTES);
    memcpy(out, PARTITION_MAGIC, 8);
    const uint32_t f[4] = {h.version, h.dim, h.n_lists, h.n_part};
    for (int i = 0; i < 4; ++i) put_u32(out + 8 + 4 * i, f[i]);
}

bool partition_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, PartitionFileHeader &h, std::string &err) {
    const unsigned char *p = (const unsigned char *)buf;
    if (!p || buf_len < INDEX_HEADER_BYTES) { err = "shorter than the 64-byte header"; return false; }
    if (memcmp(p, PARTITION_MAGIC, 8) != 0) { err = "not a partition file (magic BHIPPRT1 expected)"; return false; }
    PartitionFileHeader g;
    g.version = get_u32(p + 8); g.dim = get_u32(p + 12); g.n_lists = get_u32(p + 16); g.n_part = get_u32(p + 20);
    if (g.version != PARTITION_FILE_VERSION) { err = "version " + std::to_string(g.version) + " (this build reads version 1)"; return false; }
    if (g.dim < 1 || g.dim > (uint32_t)INDEX_MAX_DIM) { err = "dim " + std::to_string(g.dim) + " (1 .. 2048)"; return false; }
    if (g.n_lists < 1 || g.n_lists > PARTITION_MAX_LISTS) { err = "n_lists " + std::to_string(g.n_lists) + " (1 .. 65536)"; return false; }
    if (g.n_part > 0x7fffffffu) { err = "more than 2^31 - 1 assigned rows"; return false; }
    for (size_t i = 24; i < INDEX_HEADER_BYTES; ++i)
        if (p[i]) { err = "non-zero reserved header bytes"; return false; }
    const uint64_t want = partition_file_bytes(g);
    if (file_bytes != want) {
        err = "the file has " + std::to_string(file_bytes) + " bytes, its header describes " + std::to_string(want) +
              (file_bytes < want ? " (truncated)" : " (over-long)");
        return false;
    }
    h = g;
    return true;
}

}  // namespace bert_hip
