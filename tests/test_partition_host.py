"""The cluster partition of the embedding index without a GPU: the new entry points refuse a missing index instead of crashing,
and the list builder (partition.h build_lists, through libbert_test.so's bert_hip_test_build_lists) equals a stable sort."""
import ctypes as C

import numpy as np
import pytest

from bert_cpp_amd import pybert


def test_partition_entry_points_refuse_a_missing_index(sparse_vocab_model, capfd):
    m = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    try:
        L = m.lib
        assert not L.bert_hip_index_create(m.ctx, 0, 1)                  # (a tokenizer-only context holds no index)
        ids = np.zeros(4, np.int32)
        f = np.full(8, 0.5, np.float32)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        pi, pf = ids.ctypes.data_as(i32p), f.ctypes.data_as(f32p)
        capfd.readouterr()
        assert L.bert_hip_index_n_lists(None) == -1
        assert L.bert_hip_index_get_rows(None, 1, pi, pf) == -1
        assert L.bert_hip_index_partition(None, 1, pf) == -1
        assert L.bert_hip_index_partition(None, 0, None) == -1
        assert L.bert_hip_index_partition_centroids(None, pf) == -1
        assert L.bert_hip_index_partition_lists(None, pi) == -1
        assert L.bert_hip_index_kmeans(None, 1, 1, pf) == -1
        assert L.bert_hip_index_search_probed(None, 1, pf, 1, 1, pi, pf) == -1
        assert L.bert_hip_index_search_probed_device(None, 1, None, 1, 1, None, None, None) == -1
        err = capfd.readouterr().err
        for name in ("get_rows", "partition", "partition_centroids", "partition_lists", "kmeans", "search_probed", "search_probed_device"):
            assert f"bert_hip_index_{name}: no index" in err, name
        assert (ids == 0).all() and (f == 0.5).all()
    finally:
        m.close()


def build_lists(list_of, n_lists):
    L = pybert.test_lib()
    list_of = np.ascontiguousarray(list_of, dtype=np.int32)
    offsets = np.full(n_lists + 1, -7, np.int32)
    order = np.full(max(len(list_of), 1), -7, np.int32)
    i32p = C.POINTER(C.c_int32)
    n = L.bert_hip_test_build_lists(list_of.ctypes.data_as(i32p), len(list_of), n_lists, offsets.ctypes.data_as(i32p), order.ctypes.data_as(i32p))
    assert n >= 0
    assert (order[n:] == -7).all()
    return offsets, order[:n]


@pytest.mark.parametrize("n,n_lists,holes", [(0, 3, False), (1, 1, False), (1000, 12, False), (1000, 12, True), (5000, 700, True), (257, 65536, True)])
def test_build_lists_is_a_stable_sort_by_list(n, n_lists, holes):
    rng = np.random.default_rng(n + n_lists)
    list_of = rng.integers(0, n_lists, n).astype(np.int32)
    if n_lists >= 12:
        list_of[list_of == 7] = 3                                        # an empty list in the middle
        list_of[list_of == n_lists - 1] = 0                              # and at the end
    if holes:
        list_of[rng.random(n) < 0.2] = -1                                # unassigned rows are in no list
        list_of[-40:] = -1                                               # (a tail)
    offsets, order = build_lists(list_of, n_lists)
    rows = np.nonzero(list_of >= 0)[0]
    want = rows[np.argsort(list_of[rows], kind="stable")].astype(np.int32)
    assert np.array_equal(order, want)
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(np.bincount(list_of[rows], minlength=n_lists))]).astype(np.int32))
    assert offsets[-1] == len(rows)


def test_build_lists_ignores_ids_beyond_the_lists_and_rejects_bad_arguments():
    offsets, order = build_lists(np.array([2, 5, 0, -3, 2, 3, 0], np.int32), 3)
    assert offsets.tolist() == [0, 2, 2, 4] and order.tolist() == [2, 6, 0, 4]
    L = pybert.test_lib()
    assert L.bert_hip_test_build_lists(None, 3, 2, None, None) == -1
    assert L.bert_hip_test_build_lists(None, -1, 2, None, None) == -1
