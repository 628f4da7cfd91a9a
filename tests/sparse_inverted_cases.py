"""The search cases of the sparse index's inverted search (bert_hip.h "Sparse index: postings and the inverted search"), shared by
tests/test_sparse_inverted_host.py (the reference-only guard), tests/test_gpu_sparse_inverted.py and, for case "a" at ROWS_SLICED rows,
tests/test_gpu_sparse_inverted_order.py and tests/test_sparse_inverted_order_host.py.  Rows and queries come from the
generators of tests/test_gpu_sparse_index.py; the reference (tests/sparse_index_reference.py) is computed once per (case, dtype, rows)
and never changed.  No GPU, no library."""
import numpy as np

import sparse_index_reference as ref
from test_gpu_sparse_index import _terms, _weights  # noqa: F401  (the generators the row-major tests use)

NQ = 70
SEG_TEST = 256          # "sparse_index_segment_rows" of the tests: 700 rows are three segments, the last one partial, ending inside a block of 64
SEG_DEFAULT = 2048      # the built-in segment size (sparse_index_kernels.h SPARSE_SEGMENT_ROWS)
ROWS = 700
ABSENT = (7, 11)        # ids no row of a case holds: query 4 asks for exactly these
# case "a" enlarged (tests/test_gpu_sparse_inverted_order.py): 11 segments of SEG_TEST rows, the last of 130, and the NQ queries TILING
# times over — 525 tiles of two, for which the plan cuts slices of 3, 3, 3 and 2 segments (test_sparse_inverted_order_host.py)
ROWS_SLICED = 2690
TILING = 15

# name: (V, dtypes, width, row fill, rows, kq, query fill, skew)
CASES = {
    "a": (1000, ("f32", "f16"), 128, 128, ROWS, 32, 32, 2.0),
    "b": (40, ("f32", "f16"), 40, 40, ROWS, 40, 40, 1.0),                # every list holds most of the segment
    "c": (30522, ("f32", "f16"), 128, 100, ROWS, 256, 256, 3.0),
    "c_default_seg": (30522, ("f32", "f16"), 128, 100, 2 * SEG_DEFAULT + 130, 256, 256, 3.0),
    "d": (30522, ("f32", "f16"), 5, 5, ROWS, 32, 32, 1.0),               # most rows score +0: ties by id
    "e": (65536, ("f16",), 64, 64, ROWS, 32, 32, 2.0),                   # id 65535 stored and queried
    "f": (65537, ("f32",), 32, 32, ROWS, 32, 32, 2.0),
    "g": (262144, ("f32",), 256, 256, 130, 256, 256, 3.0),
    "h": (1000, ("f32", "f16"), 128, 128, 1, 32, 32, 2.0),               # one row (the full one)
}
# the cases whose rows share enough terms with a query for the order of the chain to show in the bits
CHAIN_CASES = ("a", "b", "c", "c_default_seg")

_DATA = {}
_SCORES = {}


def data(name, rows=None):
    """(ids, w, q_ids, q_w) of a case: query 0 has only -1s, query 3 asks for the vocabulary's last id, which row 3 stores, query 4 asks
    for ABSENT alone, which no row holds"""
    V, _, width, fill, n, kq, qfill, skew = CASES[name]
    n = n if rows is None else rows
    if (name, n) in _DATA:
        return _DATA[(name, n)]
    rng = np.random.default_rng(sum(map(ord, name)) + V)
    ids, w = _terms(rng, max(n, 3), width, V, fill, skew)
    ids, w = ids[-n:], w[-n:]
    q_ids, q_w = _terms(rng, NQ, kq, V, qfill, skew)
    if V > 40:
        ids[np.isin(ids, ABSENT)] = -1
        q_ids[4] = -1
        q_ids[4, :len(ABSENT)] = ABSENT
    if n > 3 and width > 1:
        ids[3], q_ids[3] = -1, -1
        ids[3, :2], q_ids[3, 0] = [V - 1, 0], V - 1
    _DATA[(name, n)] = (ids, w, q_ids, q_w)
    return _DATA[(name, n)]


def scores(name, dtype, rows=None, descending=False):
    """the reference's scores [NQ][rows] of a case; descending: the chain evaluated in DESCENDING id instead (the guard's control)"""
    V, _, width = CASES[name][:3]
    ids, w, q_ids, q_w = data(name, rows)
    key = (name, dtype, len(ids), descending)
    if key not in _SCORES:
        st_i, st_w = ref.stored_rows(ids, w, width, dtype)
        if descending:
            st_i, st_w = st_i[:, ::-1], st_w[:, ::-1]            # (scores walks the columns in order and skips the -1s)
        sc = ref.scores(st_i, st_w, q_ids, q_w, V)
        sc.setflags(write=False)
        _SCORES[key] = sc
    return _SCORES[key]


def want(sc, k, qualifies=None):
    """the reference's top-k of every query over the rows that qualify (a bool array, None = all)"""
    res = []
    for s in sc:
        if qualifies is not None:
            s = np.where(qualifies, s, np.float32(np.nan))      # (a NaN score is never returned)
        res.append(ref.topk(s, k))
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
