// token_index_file.h — the file form of a token index (bert_hip_late_index_save / _load; the format is stated in include/bert_hip.h).
// Plain host C++, as sparse_index_file.h: the 64-byte header, the length it describes, and the checks a file passes in front of a
// load — the header against the file's length before anything is allocated, then the body: cumulative lengths, live words.  The check
// of the cumulative lengths is what keeps the scan's row reads inside the stored rows.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "index_file.h"

namespace bert_hip {

constexpr uint32_t TOKEN_INDEX_FILE_VERSION = 1;
constexpr uint32_t TOKEN_FILE_MAX_DIM = 1024;

struct TokenIndexFileHeader {
    uint32_t version = TOKEN_INDEX_FILE_VERSION, dim = 0, n_docs = 0, has_live = 0;
    uint64_t n_tokens = 0;
};

// bytes of the cumulative lengths, of the rows and of the live words of the file this header describes
inline uint64_t token_index_file_cu_bytes(const TokenIndexFileHeader &h) { return ((uint64_t)h.n_docs + 1) * 4; }
inline uint64_t token_index_file_row_bytes(const TokenIndexFileHeader &h) { return h.n_tokens * (uint64_t)h.dim * 2; }
inline uint64_t token_index_file_live_bytes(const TokenIndexFileHeader &h) { return h.has_live ? ((uint64_t)h.n_docs + 31) / 32 * 4 : 0; }
// the length of the file: header, lengths, rows, live words (64-bit: 2^31 - 1 rows of 1024 halfs need 42 bits of bytes)
uint64_t token_index_file_bytes(const TokenIndexFileHeader &h);
void token_index_header_write(const TokenIndexFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]);
// Parses and checks the first buf_len bytes of a file of file_bytes bytes: magic, version 1, dim a multiple of 8 in 8 .. 1024,
// n_tokens < 2^31, n_docs <= n_tokens, has_live 0 or 1, reserved bytes zero, and file_bytes exactly token_index_file_bytes.
// false + err otherwise.
bool token_index_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, TokenIndexFileHeader &h, std::string &err);

// cu [n_docs + 1]: cu[0] == 0, strictly ascending, cu[n_docs] == n_tokens
bool token_index_cu_check(const TokenIndexFileHeader &h, const int32_t *cu, std::string &err);
// no bit at or beyond n_docs set in words [ceil(n_docs / 32)]
bool token_index_live_check(const TokenIndexFileHeader &h, const uint32_t *words, std::string &err);
// the two of them over a whole body (the file behind its header) in memory: body_len must be the body's length.  The rows are not
// looked at.
bool token_index_body_check(const TokenIndexFileHeader &h, const void *body, uint64_t body_len, std::string &err);

}  // namespace bert_hip
