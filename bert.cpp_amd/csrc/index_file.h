// index_file.h — the file forms of an embedding index and of its partition (bert_hip_index_save / _load, _partition_save / _load; the
// formats are stated in include/bert_hip.h).
// Plain host C++: what a stored row looks like for each dtype, the 64-byte header, and the one check a file passes before
// anything is allocated for it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace bert_hip {

constexpr size_t INDEX_HEADER_BYTES = 64;
constexpr uint32_t INDEX_FILE_VERSION = 1;
constexpr int INDEX_MAX_DIM = 2048;

// bytes per stored element of dtype 0 (f32), 1 (f16), 2 (i8); 0 for any other dtype (3, b1, stores an eighth of a byte)
int index_elem_size(int dtype);
// elements per stored row: dim rounded up to the score kernel's k-step (8 floats, 16 halves, 32 bytes) or, for dtype 3 (b1),
// to the 128 bits of a 16-byte piece
int index_dpad(int dtype, int dim);
// bytes per stored row of dpad elements: dpad * index_elem_size, dpad / 8 for dtype 3 (one bit per element)
uint64_t index_row_bytes(int dtype, int dpad);

struct IndexFileHeader {
    uint32_t version = INDEX_FILE_VERSION, dtype = 0, dim = 0, dpad = 0, n_rows = 0, has_live = 0;
};

// the length of the file this header describes: header, rows (index_row_bytes each), i8 scales, live words
uint64_t index_file_bytes(const IndexFileHeader &h);
// the header's 64 bytes, little-endian
void index_header_write(const IndexFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]);
// Parses and checks the first buf_len bytes of a file of file_bytes bytes: magic, version, dtype 0 .. 3, dim 1 .. 2048, dpad as
// index_dpad gives it, reserved bytes zero, has_live 0 or 1, and file_bytes exactly index_file_bytes.  false + err otherwise.
bool index_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, IndexFileHeader &h, std::string &err);

// The partition file (bert_hip_index_partition_save / _load), a file of its own beside the index file: a 64-byte header, then
// n_lists * dim f32 centroids, then n_part i32 list ids — the rows behind the first n_part are the tail.
constexpr uint32_t PARTITION_FILE_VERSION = 1;
constexpr uint32_t PARTITION_MAX_LISTS = 65536;

struct PartitionFileHeader {
    uint32_t version = PARTITION_FILE_VERSION, dim = 0, n_lists = 0, n_part = 0;
};

// the length of the file this header describes (64-bit: n_part alone may need 33 bits of bytes)
uint64_t partition_file_bytes(const PartitionFileHeader &h);
void partition_header_write(const PartitionFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]);
// As index_header_check, for a partition file: magic, version, dim 1 .. 2048, n_lists 1 .. 65536, n_part <= 2^31 - 1, reserved
// bytes zero, and file_bytes exactly partition_file_bytes.  false + err otherwise.
bool partition_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, PartitionFileHeader &h, std::string &err);

}  // namespace bert_hip
