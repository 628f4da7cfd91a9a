// host_chunks.h — how a host-resident packed batch is cut into chunks and how one chunk is laid out for its single copy to the
// device.  Pure host code (no HIP): the engine's host forms (engine_host.cpp) and the indexes' text routes (text_routes.h) share it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace bert_hip {

struct HostChunk { int b0, b1, max_len; };     // sentences [b0, b1) of a batch and the longest of them

// THE CHUNK RULE: the chunk that starts at sentence b0 takes sentences while they fit chunk_tokens tokens (a cut falls between
// sentences only) and, with max_sentences > 0, while there are fewer than max_sentences of them; it always takes at least one, so
// a sentence longer than chunk_tokens is a chunk of its own.  cu: the batch's prefix sums, B + 1 entries, from any origin.
inline HostChunk next_host_chunk(const int32_t *cu, int B, int b0, int chunk_tokens, int max_sentences) {
    HostChunk c{b0, b0 + 1, cu[b0 + 1] - cu[b0]};
    while (c.b1 < B && (max_sentences == 0 || c.b1 - c.b0 < max_sentences) && cu[c.b1 + 1] - cu[b0] <= chunk_tokens) {
        c.max_len = std::max(c.max_len, cu[c.b1 + 1] - cu[c.b1]);
        ++c.b1;
    }
    return c;
}

// The staging block of a chunk of T tokens in nb sentences: ids [T] | cu_seqlens [nb + 1] | first_len [nb] (a typed chunk) |
// windows [n_windows] ({first sentence, count} pairs of int32), every part at a multiple of 16 bytes; `bytes` ends at the last part's
// last byte.  A part that is absent is empty, and the next one starts where it would have.
struct StagingLayout {
    size_t off_cu, off_first_len, off_windows, bytes;
    StagingLayout(size_t T, size_t nb, bool typed, size_t n_windows) {
        auto pad16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
        off_cu = pad16(T * 4);
        off_first_len = off_cu + pad16((nb + 1) * 4);
        off_windows = typed ? off_first_len + pad16(nb * 4) : off_first_len;
        bytes = n_windows ? off_windows + n_windows * 8 : typed ? off_first_len + nb * 4 : off_cu + (nb + 1) * 4;
    }
};

// Writes chunk c of the batch (tokens, cu) into a host block of L.bytes bytes: the ids copied, cu_seqlens rebased to the chunk's
// first token, first_len (per sentence of the batch; null for an untyped layout) and the windows (null for none) where present.
// Returns the chunk's cu_seqlens in the block.
inline int32_t *fill_staging(char *block, const StagingLayout &L, const int32_t *tokens, const int32_t *cu, const HostChunk &c,
                             const int32_t *first_len, const void *windows, size_t n_windows) {
    const int nb = c.b1 - c.b0;
    memcpy(block, tokens + cu[c.b0], (size_t)(cu[c.b1] - cu[c.b0]) * 4);
    int32_t *h_cu = (int32_t *)(block + L.off_cu);
    for (int j = 0; j <= nb; ++j) h_cu[j] = cu[c.b0 + j] - cu[c.b0];
    if (first_len) memcpy(block + L.off_first_len, first_len + c.b0, (size_t)nb * 4);
    if (n_windows) memcpy(block + L.off_windows, windows, n_windows * 8);
    return h_cu;
}

}  // namespace bert_hip
