// sparse_index_file.h — the file form of a sparse index (bert_hip_sparse_index_save / _load; the format is stated in
// include/bert_hip.h).  Plain host C++, as index_file.h: the 64-byte header, the length it describes, and the checks a file passes in
// front of a load — the header against the file's length before anything is allocated, then the body: counts, used ids, live words.
// The id check is what keeps the scan's LDS reads inside a query image.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "index_file.h"

namespace bert_hip {

constexpr uint32_t SPARSE_INDEX_FILE_VERSION = 1;
constexpr uint32_t SPARSE_FILE_MAX_VOCAB = 262144, SPARSE_FILE_MAX_WIDTH = 256, SPARSE_FILE_BLOCK_ROWS = 64;

struct SparseIndexFileHeader {
    uint32_t version = SPARSE_INDEX_FILE_VERSION, dtype = 0, n_vocab = 0, width = 0, n_rows = 0, has_live = 0;
};

// bytes of a stored id and of a stored weight (dtype 0: i32 + f32, 1: u16 + f16: the two are equal)
inline uint64_t sparse_file_elem_bytes(uint32_t dtype) { return dtype == 1 ? 2 : 4; }
// bytes of one of the two block arrays: ceil(n_rows / 64) blocks of [width][64] elements
uint64_t sparse_index_file_array_bytes(const SparseIndexFileHeader &h);
// the length of the file this header describes: header, id blocks, weight blocks, counts, live words (64-bit: the blocks of 2^31 rows
// of 256 terms need 41 bits of bytes)
uint64_t sparse_index_file_bytes(const SparseIndexFileHeader &h);
void sparse_index_header_write(const SparseIndexFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]);
// Parses and checks the first buf_len bytes of a file of file_bytes bytes: magic, version, dtype 0 .. 1, n_vocab 1 .. 262144 (dtype 1:
// at most 65536), width 1 .. 256, n_rows at most 2^31 - 65, has_live 0 or 1, reserved bytes zero, and file_bytes exactly
// sparse_index_file_bytes.  false + err otherwise.
bool sparse_index_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, SparseIndexFileHeader &h, std::string &err);

// every count in [0, width]
bool sparse_index_counts_check(const SparseIndexFileHeader &h, const int32_t *counts, std::string &err);
// ids: n_blocks blocks of [width][64] stored ids, the index's blocks first_block ...; every id in a column below its row's count (counts:
// all n_rows of them, checked) is below n_vocab.  Rows at or beyond n_rows, and columns at or behind a count, are not looked at.
bool sparse_index_ids_check(const SparseIndexFileHeader &h, const void *ids, uint64_t first_block, uint64_t n_blocks, const int32_t *counts,
                            std::string &err);
// no bit at or beyond n_rows set in words [ceil(n_rows / 32)]
bool sparse_index_live_check(const SparseIndexFileHeader &h, const uint32_t *words, std::string &err);
// the three of them over a whole body (the file behind its header) in memory: body_len must be the body's length
bool sparse_index_body_check(const SparseIndexFileHeader &h, const void *body, uint64_t body_len, std::string &err);

}  // namespace bert_hip
