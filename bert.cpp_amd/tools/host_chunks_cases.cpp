// host_chunks_cases.cpp — host_chunks.h's staging layout and fill under the sanitizers (make check-host): every shape's block is
// allocated at exactly `bytes`, so a write past a part's end or the block's is an error; the parts' offsets are 16-byte aligned and
// do not overlap, the ids, first_len and windows arrive unchanged and cu_seqlens rebased to the chunk's first token.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_chunks.h"

using namespace bert_hip;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (T %d, nb %d, typed %d, windows %d)\n", __FILE__, __LINE__, #c, T, nb, (int)typed, n_windows); ++failures; } } while (0)

int main() {
    int shapes = 0;
    for (int T : {1, 3, 4, 5})
        for (int nb : {1, 2})
            for (bool typed : {false, true})
                for (int n_windows : {0, nb}) {
                    if (nb > T) continue;
                    // the chunk is sentences [1, 1 + nb) of a batch whose prefix sums start at 100 (the ids are indexed by them): a sentence of 9 tokens in front of it
                    std::vector<int32_t> cu = {100, 109};
                    for (int j = 0; j < nb; ++j) cu.push_back(j + 1 < nb ? cu.back() + 1 : 109 + T);
                    std::vector<int32_t> tokens(109 + T), first_len(1 + nb), windows(2 * nb);
                    for (size_t i = 0; i < tokens.size(); ++i) tokens[i] = 1000 + (int32_t)i;
                    for (size_t i = 0; i < first_len.size(); ++i) first_len[i] = 50 + (int32_t)i;
                    for (size_t i = 0; i < windows.size(); ++i) windows[i] = 70 + (int32_t)i;
                    const HostChunk c = next_host_chunk(cu.data(), 1 + nb, 1, 1 << 20, 0);
                    CHECK(c.b0 == 1 && c.b1 == 1 + nb);
                    const StagingLayout L((size_t)T, (size_t)nb, typed, (size_t)n_windows);
                    const size_t end_ids = (size_t)T * 4, end_cu = L.off_cu + (size_t)(nb + 1) * 4, end_fl = L.off_first_len + (typed ? (size_t)nb * 4 : 0),
                                 end_w = L.off_windows + (size_t)n_windows * 8;
                    CHECK(L.off_cu % 16 == 0 && L.off_first_len % 16 == 0 && L.off_windows % 16 == 0);
                    CHECK(end_ids <= L.off_cu && end_cu <= L.off_first_len && end_fl <= L.off_windows);
                    CHECK(L.bytes == (n_windows ? end_w : typed ? end_fl : end_cu));
                    char *block = (char *)malloc(L.bytes);
                    const int32_t *h_cu = fill_staging(block, L, tokens.data(), cu.data(), c, typed ? first_len.data() : nullptr, windows.data(), (size_t)n_windows);
                    CHECK((const char *)h_cu == block + L.off_cu);
                    for (int t = 0; t < T; ++t) CHECK(((const int32_t *)block)[t] == 1109 + t);
                    for (int j = 0; j <= nb; ++j) CHECK(h_cu[j] == cu[1 + j] - 109);
                    CHECK(h_cu[0] == 0 && h_cu[nb] == T);
                    for (int j = 0; typed && j < nb; ++j) CHECK(((const int32_t *)(block + L.off_first_len))[j] == 51 + j);
                    for (int j = 0; j < 2 * n_windows; ++j) CHECK(((const int32_t *)(block + L.off_windows))[j] == 70 + j);
                    free(block);
                    ++shapes;
                }
    printf("host_chunks_cases: %d shapes, %d failures\n", shapes, failures);
    return failures ? 1 : 0;
}
