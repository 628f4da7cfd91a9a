// partition.h — the list tables of a cluster partition of an embedding index (search.h), built on the host from one list id per
// row.  No device code: the Index uploads what this returns (index_partition.cpp), and a test reaches it without a device.
#pragma once
#include <cstdint>
#include <vector>

namespace bert_hip {

// offsets [n_lists + 1], order [offsets[n_lists]]: the members of list l are order[offsets[l] .. offsets[l + 1]), row ids in
// ascending order
struct ListTables {
    std::vector<int32_t> offsets, order;
};

// A stable counting sort of the rows 0 .. n - 1 by list_of[row]; rows whose entry is outside [0, n_lists) (-1: unassigned, or
// left out by the caller) are in no list.
void build_lists(const int32_t *list_of, int n, int n_lists, ListTables &t);

}  // namespace bert_hip
