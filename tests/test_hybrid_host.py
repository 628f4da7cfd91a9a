"""Host tests of the hybrid search (include/bert_hip.h "Hybrid search"): how a call is chunked (bert_hip_test_hybrid_chunk, the function
the search itself calls), the reference's score rule against an fma, the exported names and the binding.  No GPU."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

import hybrid_reference as href
import sparse_index_reference as sref
from conftest import ROOT

NEW_SYMBOLS = ["bert_hip_hybrid_reserve", "bert_hip_hybrid_search", "bert_hip_hybrid_search_device", "bert_hip_hybrid_search_texts"]
HOOK = "bert_hip_test_hybrid_chunk"
MIB256 = 256 << 20

ROWS = [1, 64, 65, 10 ** 6, 7 * 10 ** 7]
QUERIES = [1, 31, 33, 4096, 5000]
PREFS = [0, 1, 3, 40]


# (n_rows, nq, pref) -> (HC, ld), worked out by hand from the rule of the header
TABLE = {
    (1, 1, 0): (1, 64),
    (1, 5000, 0): (4096, 64),                    # 4096 x 64 floats = 1 MiB: the indexes' own chunk is the limit
    (64, 31, 0): (31, 64),                       # fewer than 32: as many as there are
    (64, 33, 0): (32, 64),                       # 33 would leave a dense tile of one query in every chunk: 32, then 1
    (65, 33, 0): (32, 128),                      # ld rounds up to 64 floats
    (65, 33, 40): (33, 128),                     # forced: not rounded, and never more than nq
    (65, 4096, 3): (3, 128),
    (10 ** 6, 4096, 0): (64, 10 ** 6),           # 256 MiB / 4 MB = 67 queries, rounded down to 64
    (10 ** 6, 5000, 40): (40, 10 ** 6),
    (10 ** 6, 31, 40): (31, 10 ** 6),
    (10 ** 6, 4096, 1): (1, 10 ** 6),
    (7 * 10 ** 7, 5000, 0): (1, 7 * 10 ** 7),    # one query's scores are 280 MB: taken whatever they need
    (7 * 10 ** 7, 5000, 40): (1, 7 * 10 ** 7),   # a forced chunk stays under the workspace's bound
}


def test_the_chunk_hook_against_a_table():
    for args, want in TABLE.items():
        assert pybert.test_hybrid_chunk(*args) == want, args
        assert href.chunk_queries(*args) == want, args
    for n in ROWS:
        for nq in QUERIES:
            for pref in PREFS:
                assert pybert.test_hybrid_chunk(n, nq, pref) == href.chunk_queries(n, nq, pref), (n, nq, pref)


def test_the_chunk_hook_keeps_its_invariants():
    for n in ROWS + [0, 63, 2 ** 31 - 65]:
        for nq in QUERIES:
            for pref in PREFS:
                hc, ld = pybert.test_hybrid_chunk(n, nq, pref)
                assert ld % 64 == 0 and n <= ld < n + 64, (n, ld)
                assert 1 <= hc <= min(nq, 4096), (n, nq, pref, hc)
                assert hc * ld * 4 <= MIB256 or hc == 1, (n, nq, pref, hc)
                if pref == 0 and hc >= 32:
                    assert hc % 32 == 0, (n, nq, hc)
                if pref > 0:
                    assert hc <= pref
                # unforced: no larger chunk would do
                if pref == 0 and hc < min(nq, 4096) and hc >= 32:
                    assert (hc + 32) * ld * 4 > MIB256 or hc + 32 > min(nq, 4096), (n, nq, hc)
    T = pybert.test_lib()
    assert T.bert_hip_test_hybrid_chunk(10, 1, 0, None) == -1
    for bad in ((-1, 1, 0), (10, 0, 0), (10, 1, -1)):
        assert pybert.test_hybrid_chunk(*bad) is None, bad


def test_the_rule_is_two_products_and_a_sum_not_an_fma():
    """wd D = 1 + 2^-11 + 2^-24 exactly: rounded on its own it is 1 + 2^-11 (a tie, to even), and adding ws S = 2^-24 is a tie again:
    1 + 2^-11.  An fma keeps the product exact: 1 + 2^-11 + 2^-23, the next float."""
    wd = D = np.float32(1 + 2.0 ** -12)
    ws, S = np.float32(1.0), np.float32(2.0 ** -24)
    rule = href.combine(np.array([D]), np.array([S]), wd, ws)[0]
    fused = sref.fma_f32(wd, D, ws * S)
    assert rule == np.float32(1 + 2.0 ** -11) and fused == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert int(fused.view(np.uint32)) - int(rule.view(np.uint32)) == 1
    # the rule over arrays is the rule per element, and NaN / inf pass through it
    D2 = np.array([[D, np.nan, np.inf, -1.5]], np.float32)
    S2 = np.array([[S, 1.0, 1.0, 0.0]], np.float32)
    H = href.combine(D2, S2, wd, ws)
    assert H.dtype == np.float32 and H[0, 0] == rule and np.isnan(H[0, 1]) and np.isposinf(H[0, 2]) and H[0, 3] == np.float32(wd * np.float32(-1.5))
    ids, sc = href.search(D2, S2, np.array([True, True, True, False]), wd, ws, 4)
    assert ids.tolist() == [[2, 0, -1, -1]] and np.isposinf(sc[0, 0]) and sc[0, 1] == rule and np.isneginf(sc[0, 2:]).all()
    # (0, 0): every finite score is a zero, and the smallest ids win
    ids, sc = href.search(np.array([[3.0, 1.0, 2.0]], np.float32), np.array([[1.0, 0.0, 5.0]], np.float32), np.ones(3, bool), 0.0, 0.0, 2)
    assert ids.tolist() == [[0, 1]] and (sc == 0).all() and not np.signbit(sc).any()


def test_new_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    declared = set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", text))
    exported = {p: subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout.split()
                for p in (pybert.LIB_PATH, pybert.TEST_LIB_PATH)}
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in pybert.BERT_HIP_H_SYMBOLS, sym
        assert sym in exported[pybert.LIB_PATH] and sym in exported[pybert.TEST_LIB_PATH], sym
    assert "Hybrid search" in text and '"hybrid_chunk_queries"' in text
    test_text = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    assert re.search(r"BERT_API int32_t " + HOOK + r"\(", test_text) and HOOK in pybert.BERT_HIP_TEST_H_SYMBOLS and HOOK not in text
    assert HOOK in exported[pybert.TEST_LIB_PATH] and HOOK not in exported[pybert.LIB_PATH]
    assert not any("hybrid" in s and s not in NEW_SYMBOLS + [HOOK] for s in exported[pybert.TEST_LIB_PATH])


def test_binding_has_the_new_methods_with_the_issues_defaults():
    sig = inspect.signature(pybert.BertIndex.hybrid_search)
    assert list(sig.parameters)[:5] == ["self", "sparse", "queries", "q_ids", "q_weights"]
    assert (sig.parameters["k"].default, sig.parameters["w_dense"].default, sig.parameters["w_sparse"].default, sig.parameters["allow"].default) == (10, 1.0, 1.0, None)
    sig = inspect.signature(pybert.BertIndex.hybrid_search_texts)
    assert (sig.parameters["kq"].default, sig.parameters["k"].default) == (32, 10)
    for name in ("hybrid_search_device", "hybrid_reserve"):
        assert callable(getattr(pybert.BertIndex, name)), name
    L = pybert.lib()
    # the weights travel as C floats
    import ctypes as C
    assert L.bert_hip_hybrid_search.argtypes[7:9] == [C.c_float, C.c_float]
    assert L.bert_hip_hybrid_search_device.argtypes[7:9] == [C.c_float, C.c_float]
    assert L.bert_hip_hybrid_search_texts.argtypes[6:8] == [C.c_float, C.c_float]


def test_entry_points_refuse_missing_indexes(capfd):
    """-1 after a line on stderr without one of the indexes: nothing touches a device"""
    L = pybert.lib()
    capfd.readouterr()
    assert L.bert_hip_hybrid_reserve(None, None, 10, 1, 1) == -1
    assert "bert_hip_hybrid_reserve" in capfd.readouterr().err
    out_i, out_s = np.full(4, 7, np.int32), np.full(4, 7.0, np.float32)
    assert L.bert_hip_hybrid_search(None, None, 1, None, 1, None, None, 1.0, 1.0, None, 0, 4, out_i.ctypes.data, out_s.ctypes.data) == -1
    assert L.bert_hip_hybrid_search_device(None, None, 1, None, 1, None, None, 1.0, 1.0, None, 0, 4, out_i.ctypes.data, out_s.ctypes.data, None) == -1
    assert L.bert_hip_hybrid_search_texts(None, None, 1, 1, None, 4, 1.0, 1.0, 4, out_i.ctypes.data, out_s.ctypes.data) == -1
    assert capfd.readouterr().err.count("no embedding index") == 3
    assert (out_i == 7).all() and (out_s == 7.0).all()
