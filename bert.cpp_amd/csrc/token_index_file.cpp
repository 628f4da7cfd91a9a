// token_index_file.cpp — header and body checks of a token index file (token_index_file.h).  No device, no alignment assumed.
#include "token_index_file.h"

#include <cstring>

#include "live_bits.h"

namespace bert_hip {

namespace {

const char TOKEN_MAGIC[8] = {'B', 'H', 'I', 'P', 'T', 'O', 'K', '1'};

void put_u32(unsigned char *p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (8 * i));
}

uint32_t get_u32(const unsigned char *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

}  // namespace

uint64_t token_index_file_bytes(const TokenIndexFileHeader &h) {
    return INDEX_HEADER_BYTES + token_index_file_cu_bytes(h) + token_index_file_row_bytes(h) + token_index_file_live_bytes(h);
}

void token_index_header_write(const TokenIndexFileHeader &h, unsigned char out[INDEX_HEADER_BYTES]) {
    memset(out, 0, INDEX_HEADER_BYTES);
    memcpy(out, TOKEN_MAGIC, 8);
    const uint32_t f[6] = {h.version, h.dim, h.n_docs, h.has_live, (uint32_t)h.n_tokens, (uint32_t)(h.n_tokens >> 32)};
    for (int i = 0; i < 6; ++i) put_u32(out + 8 + 4 * i, f[i]);
}

bool token_index_header_check(const void *buf, size_t buf_len, uint64_t file_bytes, TokenIndexFileHeader &h, std::string &err) {
    const unsigned char *p = (const unsigned char *)buf;
    if (!p || buf_len < INDEX_HEADER_BYTES) { err = "shorter than the 64-byte header"; return false; }
    if (memcmp(p, TOKEN_MAGIC, 8) != 0) { err = "not a token index file (magic BHIPTOK1 expected)"; return false; }
    TokenIndexFileHeader g;
    g.version = get_u32(p + 8); g.dim = get_u32(p + 12); g.n_docs = get_u32(p + 16); g.has_live = get_u32(p + 20);
    g.n_tokens = (uint64_t)get_u32(p + 24) | (uint64_t)get_u32(p + 28) << 32;
    if (g.version != TOKEN_INDEX_FILE_VERSION) { err = "version " + std::to_string(g.version) + " (this build reads version 1)"; return false; }
    if (g.dim < 8 || g.dim > TOKEN_FILE_MAX_DIM || g.dim % 8) { err = "dim " + std::to_string(g.dim) + " (a multiple of 8 in 8 .. 1024)"; return false; }
    if (g.n_tokens > 0x7fffffffull) { err = "2^31 or more tokens"; return false; }
    if (g.n_docs > g.n_tokens) { err = std::to_string(g.n_docs) + " documents of " + std::to_string(g.n_tokens) + " tokens in all (no document is empty)"; return false; }
    if (g.has_live > 1) { err = "has_live " + std::to_string(g.has_live) + " (0 or 1)"; return false; }
    for (size_t i = 32; i < INDEX_HEADER_BYTES; ++i)
        if (p[i]) { err = "non-zero reserved header bytes"; return false; }
    const uint64_t want = token_index_file_bytes(g);
    if (file_bytes != want) {
        err = "the file has " + std::to_string(file_bytes) + " bytes, its header describes " + std::to_string(want) +
              (file_bytes < want ? " (truncated)" : " (over-long)");
        return false;
    }
    h = g;
    return true;
}

bool token_index_cu_check(const TokenIndexFileHeader &h, const int32_t *cu, std::string &err) {
    const unsigned char *p = (const unsigned char *)cu;
    uint32_t prev = get_u32(p);
    if (prev != 0) { err = "the cumulative lengths start at " + std::to_string((int32_t)prev) + ", not 0"; return false; }
    for (uint64_t d = 1; d <= h.n_docs; ++d) {
        const uint32_t c = get_u32(p + 4 * d);
        // (as unsigned: a negative entry is a huge one, and the last entry's check bounds them all)
        if (c <= prev || c > h.n_tokens) {
            err = "document " + std::to_string(d - 1) + " ends at " + std::to_string((int32_t)c) + " after " + std::to_string((int32_t)prev) +
                  " (strictly ascending, at most " + std::to_string(h.n_tokens) + ")";
            return false;
        }
        prev = c;
    }
    if (prev != h.n_tokens) { err = "the cumulative lengths end at " + std::to_string(prev) + ", the header says " + std::to_string(h.n_tokens) + " tokens"; return false; }
    return true;
}

bool token_index_live_check(const TokenIndexFileHeader &h, const uint32_t *words, std::string &err) {
    if (!h.has_live || (h.n_docs & 31) == 0) return true;
    const uint32_t last = get_u32((const unsigned char *)words + 4 * (uint64_t)(h.n_docs >> 5));
    if (!live_tail_clear(last, h.n_docs)) { err = "live bits beyond the last document"; return false; }
    return true;
}

bool token_index_body_check(const TokenIndexFileHeader &h, const void *body, uint64_t body_len, std::string &err) {
    if (!body || body_len != token_index_file_bytes(h) - INDEX_HEADER_BYTES) { err = "the body's length is not what the header describes"; return false; }
    const unsigned char *p = (const unsigned char *)body;
    return token_index_cu_check(h, (const int32_t *)p, err) &&
           token_index_live_check(h, (const uint32_t *)(p + token_index_file_cu_bytes(h) + token_index_file_row_bytes(h)), err);
}

}  // namespace bert_hip
