// index_io.h — the file frame of the three indexes' save and load (index_io.cpp): device memory to and from a file in pieces
// through a host buffer, never a host copy of the whole, and the atomic write of a file.  The formats are the indexes' own
// (index_file.h, sparse_index_file.h, token_index_file.h).
#pragma once
#include <cstddef>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

namespace bert_hip {

// `bytes` of device memory d <-> f at its position, in pieces of at most `piece` bytes through buf (grown as needed); blocking.
// false + err: "write failed" / "read failed", or the device's error
bool device_to_file(FILE *f, const void *d, size_t bytes, size_t piece, std::vector<char> &buf, std::string &err);
bool file_to_device(FILE *f, void *d, size_t bytes, size_t piece, std::vector<char> &buf, std::string &err);

// path written whole or not at all: body(f) writes into "<path>.tmp", which a clean close renames to path; on any failure the .tmp is
// unlinked and err, where body left it empty, becomes "cannot write '<path>'"
bool write_atomically(const char *path, std::string &err, const std::function<bool(FILE *)> &body);

}  // namespace bert_hip
