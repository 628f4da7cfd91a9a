// partition.cpp — partition.h: rows grouped by list, a pure function of the per-row list ids.
#include "partition.h"

namespace bert_hip {

void build_lists(const int32_t *list_of, int n, int n_lists, ListTables &t) {
    t.offsets.assign((size_t)n_lists + 1, 0);
    for (int r = 0; r < n; ++r)
        if (list_of[r] >= 0 && list_of[r] < n_lists) ++t.offsets[(size_t)list_of[r] + 1];
    for (int l = 0; l < n_lists; ++l) t.offsets[(size_t)l + 1] += t.offsets[l];
    t.order.assign((size_t)t.offsets[n_lists], 0);
    // (rows are visited in id order, so each list's members come out ascending)
    std::vector<int32_t> next(t.offsets.begin(), t.offsets.end() - 1);
    for (int r = 0; r < n; ++r)
        if (list_of[r] >= 0 && list_of[r] < n_lists) t.order[(size_t)next[list_of[r]]++] = r;
}

}  // namespace bert_hip
