"""Host tests of the sparse index's postings and inverted search (bert_hip.h "Sparse index: postings and the inverted search"): the
ABI's symbols, the entry points without an index, the plan of the inverted scan (sparse_index_kernels.h sparse_postings_geometry
through its test hook), and a reference-only guard that the GPU cases can see a wrong chain order at all.  No GPU."""
import os
import re

import numpy as np
import pytest

from bert_cpp_amd import pybert

import sparse_inverted_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bert_hip_sparse_index_invert", "bert_hip_sparse_index_inverted_rows", "bert_hip_sparse_index_search_inverted",
       "bert_hip_sparse_index_search_inverted_device", "bert_hip_sparse_index_search_inverted_texts"]
HOOKS = ["bert_hip_test_sparse_postings_geometry", "bert_hip_test_sparse_postings_segment"]
SPARSE_LDS_MAX = 160 * 1024 - 256       # sparse_index_kernels.h


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    test_header = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    assert "Sparse index: postings and the inverted search" in header
    lib, tlib = pybert.lib(), pybert.test_lib()
    for sym in NEW:
        assert re.search(r"BERT_API int32_t %s\(" % sym, header), sym
        assert sym in pybert.BERT_HIP_H_SYMBOLS and hasattr(lib, sym) and hasattr(tlib, sym), sym
        assert getattr(lib, sym).argtypes is not None, sym
    for sym in HOOKS:
        assert re.search(r"BERT_API int32_t %s\(" % sym, test_header), sym
        assert sym in pybert.BERT_HIP_TEST_H_SYMBOLS and hasattr(tlib, sym) and not hasattr(lib, sym), sym
    for name in ("invert", "inverted_rows", "search_inverted", "search_inverted_device", "search_texts_inverted"):
        assert hasattr(pybert.BertSparseIndex, name), name
    # the "not covered" sentences no longer name it
    for path in ("include/bert_hip.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, path)).read()
        assert not re.search(r"(Not covered|Out of scope)[^.]*[Ii]nverted|An inverted\s+\(term-major\) organisation[^.]*not covered", text), path


def test_every_entry_point_returns_minus_one_without_an_index(capfd):
    L = pybert.lib()
    buf = np.zeros((1, 4), np.int32)
    p = buf.ctypes.data
    capfd.readouterr()
    assert L.bert_hip_sparse_index_invert(None) == -1
    assert L.bert_hip_sparse_index_inverted_rows(None) == -1
    assert L.bert_hip_sparse_index_search_inverted(None, 1, 4, p, p, 1, None, 0, p, p) == -1
    assert L.bert_hip_sparse_index_search_inverted_device(None, 1, 4, p, p, 1, None, 0, p, p, None) == -1
    assert L.bert_hip_sparse_index_search_inverted_texts(None, 1, 0, None, 4, 1, p, p) == -1
    assert capfd.readouterr().err.count("no index") == 4         # (inverted_rows, like size, says nothing)
    assert not buf.any()


# (dtype, V, rows, nq, k, SEG)
PLAN_TABLE = [
    (0, 1000, 0, 1, 10, 8192),
    (0, 1000, 0, 70, 256, 256),
    (1, 30522, 8192, 1, 10, 8192), (1, 30522, 8193, 1, 10, 8192), (0, 30522, 8191, 64, 100, 8192),
    (0, 1000, 256, 70, 1, 256), (0, 1000, 257, 70, 10, 256), (1, 1000, 700, 70, 256, 256),
    (0, 262144, 130, 70, 256, 16384), (0, 262144, 10 ** 6, 4096, 256, 16384), (0, 262144, 10 ** 6, 1, 256, 8192),
    (1, 30522, 10 ** 6, 4096, 10, 8192), (0, 30522, 10 ** 6, 4096, 100, 2048), (1, 30522, 10 ** 6, 64, 10, 4096),
    (1, 65536, 2 * 8192 + 130, 70, 10, 8192), (0, 65537, 700, 70, 129, 1024), (0, 40, 2 ** 31 - 65, 4096, 256, 16384),
    (0, 40, 2 ** 31 - 65, 1, 1, 256),
]


@pytest.mark.parametrize("entry", PLAN_TABLE, ids=[",".join(map(str, e)) for e in PLAN_TABLE])
@pytest.mark.parametrize("qb", [0, 1, 2, 8])
def test_the_plan_fits_the_lds_and_cuts_whole_segments(entry, qb):
    dtype, V, rows, nq, k, seg = entry
    g = pybert.test_sparse_postings_geometry(dtype, V, rows, nq, k, seg, qb)
    assert g is not None, entry
    n_segs = -(-rows // seg)
    L = 512 if k <= 128 else 1024
    assert g["L"] == L
    per_query = seg * 4 + 256 * 8 + L * 8 + 8
    assert 1 <= g["qb"] <= min(nq, 4, qb or 2) and g["lds"] == g["qb"] * per_query <= SPARSE_LDS_MAX, g
    assert g["n_qtiles"] == -(-nq // g["qb"])
    # slices are whole segments, cover every segment, and none is empty (an empty index is one empty slice)
    assert g["slice_segs"] >= 1 and 1 <= g["n_slices"] <= g["max_slices"], g
    assert g["n_slices"] * g["slice_segs"] >= n_segs and (g["n_slices"] - 1) * g["slice_segs"] < max(n_segs, 1), g
    # the workspace bound never falls as the rows grow
    more = pybert.test_sparse_postings_geometry(dtype, V, min(rows + seg, 2 ** 31 - 65), nq, k, seg, qb)
    assert more["max_slices"] >= g["max_slices"]


def test_the_plan_refuses_what_it_cannot_cut():
    ok = (0, 1000, 700, 70, 10, 256)
    assert pybert.test_sparse_postings_geometry(*ok) is not None
    for i, bad in ((0, 2), (0, -1), (1, 0), (1, 262145), (2, -1), (3, 0), (4, 0), (4, 257), (5, 0), (5, 128), (5, 300), (5, 16384 + 256)):
        args = list(ok)
        args[i] = bad
        assert pybert.test_sparse_postings_geometry(*args) is None, args
    assert pybert.test_sparse_postings_geometry(1, 65537, 700, 70, 10, 256) is None          # u16 ids


@pytest.mark.parametrize("name", cases.CHAIN_CASES)
def test_a_wrong_chain_order_would_show_in_the_bits(name):
    """The GPU tests compare score bits with a reference that evaluates the chain in ascending id.  That only tests the ORDER of an
    inverted walk if another order gives other bits on these very operands: with the chain in descending id, at least one row's score
    changes its bits for at least half of the queries.  (Measured on the reference alone, with these files' seeds: 62 of 70 queries in case a,
    65 in b, 63 in c at 700 rows and 64 in c at twice the default segment size plus 130 rows; the reference's scores take 0.1 to 1 s a case.)  Cases d to h are about ties, ids at the vocabulary's edge and single rows: few of their rows share
    two terms with a query, and they are not held to this."""
    dtype = cases.CASES[name][1][0]
    up, down = cases.scores(name, dtype), cases.scores(name, dtype, descending=True)
    differs = (up.view(np.uint32) != down.view(np.uint32)).any(axis=1)
    print(f"case {name}: descending order changes a score of {int(differs.sum())} of {len(differs)} queries")
    assert differs.sum() * 2 >= len(differs), int(differs.sum())
