"""Host tests of the token index (include/bert_hip.h "TOKEN INDEX"): the exported names and the binding, the entry points without an
index or a device, the plan of a scan (bert_hip_test_token_index_plan, the function the search itself calls) against its restatement
and its invariants, the reference's order rule, and bert-search's new flags.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

import token_index_reference as tref
from conftest import ROOT

NEW_SYMBOLS = ["bert_hip_token_index_" + s for s in (
    "create", "free", "size", "n_tokens", "max_query_tokens", "reserve", "add", "add_device", "add_texts", "get_doc", "search", "search_device",
    "search_texts", "rescore", "rescore_device")]
HOOK = "bert_hip_test_token_index_plan"
EXE = os.path.join(ROOT, "bert.cpp_amd", "bin", "bert-search")


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    declared = set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", text))
    exported = {p: subprocess.run(["nm", "-D", "--defined-only", p], capture_output=True, text=True).stdout.split()
                for p in (pybert.LIB_PATH, pybert.TEST_LIB_PATH)}
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in pybert.BERT_HIP_H_SYMBOLS, sym
        assert sym in exported[pybert.LIB_PATH] and sym in exported[pybert.TEST_LIB_PATH], sym
    assert "TOKEN INDEX" in text and '"token_index_slices"' in text and "struct bert_hip_token_index;" in text
    test_text = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    assert re.search(r"BERT_API int32_t " + HOOK + r"\(", test_text) and HOOK in pybert.BERT_HIP_TEST_H_SYMBOLS and HOOK not in text
    assert HOOK in exported[pybert.TEST_LIB_PATH] and HOOK not in exported[pybert.LIB_PATH]
    # every exported token-index name is one of these
    assert sorted(s for s in exported[pybert.TEST_LIB_PATH] if "token_index" in s) == sorted(NEW_SYMBOLS + [HOOK])
    for name in ("add", "add_device", "add_texts", "search", "search_device", "search_texts", "rescore", "rescore_device", "get_doc", "reserve",
                 "size", "n_tokens", "max_query_tokens"):
        assert callable(getattr(pybert.BertTokenIndex, name)), name
    assert inspect.signature(pybert.BertModel.token_index).parameters["dim"].default is None
    assert pybert.lib().bert_hip_token_index_n_tokens.restype is C.c_int64


def test_entry_points_answer_minus_one_without_an_index(capfd, sparse_vocab_model):
    """-1 after a line on stderr (create: NULL) without an index, a context or a device: nothing touches a device, outputs untouched"""
    L = pybert.lib()
    capfd.readouterr()
    assert L.bert_hip_token_index_create(None, 0) is None
    assert "bert_hip_token_index_create: no context" in capfd.readouterr().err
    tok = L.bert_hip_load_tokenizer(sparse_vocab_model.encode())
    assert tok
    assert L.bert_hip_token_index_create(tok, 64) is None
    assert "tokenizer-only" in capfd.readouterr().err
    L.bert_free(tok)
    L.bert_hip_token_index_free(None)
    assert L.bert_hip_token_index_size(None) == -1 and L.bert_hip_token_index_n_tokens(None) == -1 and L.bert_hip_token_index_max_query_tokens(None) == -1
    out_i, out_s = np.full(4, 7, np.int32), np.full(4, 7.0, np.float32)
    cu = np.array([0, 1], np.int32)
    rows = np.zeros((1, 8), np.float32)
    oi, os_, cp, rp = out_i.ctypes.data, out_s.ctypes.data, cu.ctypes.data, rows.ctypes.data
    txt = (C.c_char_p * 1)(b"hello")
    capfd.readouterr()
    calls = [L.bert_hip_token_index_reserve(None, 1, 1, 1, 32, 4),
             L.bert_hip_token_index_add(None, 1, cp, rp),
             L.bert_hip_token_index_add_device(None, 1, cp, rp, None),
             L.bert_hip_token_index_add_texts(None, 1, 1, txt),
             L.bert_hip_token_index_get_doc(None, 0, rp, 1),
             L.bert_hip_token_index_search(None, 1, cp, rp, 4, oi, os_),
             L.bert_hip_token_index_search_device(None, 1, cp, rp, 32, 4, oi, os_, None),
             L.bert_hip_token_index_search_texts(None, 1, 1, txt, 4, oi, os_),
             L.bert_hip_token_index_rescore(None, 1, cp, rp, 1, cp, 4, oi, os_),
             L.bert_hip_token_index_rescore_device(None, 1, cp, rp, 1, cp, 4, oi, os_, None)]
    assert calls == [-1] * len(calls)
    assert capfd.readouterr().err.count("no index") == len(calls)
    assert (out_i == 7).all() and (out_s == 7.0).all() and (rows == 0).all()


DOCS = [0, 1, 63, 64, 65, 10 ** 6]
NQS = [1, 2, 7, 64, 256]
PREFS = [0, 1, 2, 7, 4096]


def test_the_plan_covers_every_document_exactly_once():
    for n in DOCS:
        for nq in NQS:
            for pref in PREFS + [n if 1 <= n <= 4096 else 0]:
                got = pybert.test_token_index_plan(n, nq, pref)
                assert got == tref.plan(n, nq, pref), (n, nq, pref)
                n_slices, slice_docs = got
                ranges = tref.slices_of(n, n_slices, slice_docs)
                # consecutive, without a gap or an overlap, from 0 to n_docs; no slice but an empty index's is empty
                assert ranges[0][0] == 0 and ranges[-1][1] == n, (n, nq, pref, got)
                assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
                assert all(r1 > r0 for r0, r1 in ranges) or n == 0
                # equal counts: every slice but the last holds slice_docs documents
                assert all(r1 - r0 == slice_docs for r0, r1 in ranges[:-1])
                if pref:
                    # the key is honoured: that many slices where the documents divide into them, never more
                    assert n_slices <= min(pref, max(n, 1)) and (n_slices == pref or n % pref or n < pref), (n, nq, pref, got)
                else:
                    assert nq * n_slices <= tref.TARGET_BLOCKS + nq and (n_slices == 1 or slice_docs >= tref.MIN_SLICE_DOCS), (n, nq, got)
    # (10^6 documents: 2048 slices aimed for, 489 documents each, which 2045 slices cover)
    assert pybert.test_token_index_plan(10 ** 6, 1, 0) == (2045, 489) and pybert.test_token_index_plan(300, 1, 0) == (18, 17)
    assert pybert.test_token_index_plan(300, 1, 300) == (300, 1) and pybert.test_token_index_plan(300, 7, 7) == (7, 43)
    T = pybert.test_lib()
    assert T.bert_hip_test_token_index_plan(10, 1, 0, None) == -1
    for bad in ((-1, 1, 0), (10, 0, 0), (10, 1, -1), (10, 1, 4097)):
        assert pybert.test_token_index_plan(*bad) is None and tref.plan(*bad) is None, bad


def test_max_query_tokens_of_the_reference_meets_the_floor():
    for dim in range(8, 1025, 8):
        mq = tref.max_query_tokens(dim)
        assert mq % 32 == 0 and mq <= 128
        assert mq >= (128 if dim <= 384 else 64 if dim <= 768 else 32), (dim, mq)
        assert 64 * (dim + 8) * (mq // 32) + 8 * 512 + 16 <= 160 * 1024 - 256
    assert [tref.max_query_tokens(d) for d in (8, 384, 392, 768, 776, 1024)] == [128, 128, 128, 96, 96, 64]


def test_the_reference_order_rule():
    inf, nan = np.inf, np.nan
    S = np.array([[1.0, 3.0, 3.0, nan, -inf, 3.0, 0.0, -0.0],
                  [nan, nan, nan, nan, nan, nan, nan, nan]], np.float32)
    ids, sc = tref.search_expected(S, 4)
    assert ids.tolist() == [[1, 2, 5, 0], [-1, -1, -1, -1]]                    # ties by the smaller id; a NaN row never
    assert sc[0].tolist() == [3.0, 3.0, 3.0, 1.0] and np.isneginf(sc[1]).all()
    ids, sc = tref.search_expected(S[:1], 8)
    assert ids.tolist() == [[1, 2, 5, 0, 6, 7, 4, -1]]                         # +0 == -0: by id; -inf is a score; fewer than k rows
    assert np.isneginf(sc[0, 6:]).all()
    ids, sc = tref.search_expected(np.zeros((2, 0), np.float32), 3)            # an empty index
    assert (ids == -1).all() and np.isneginf(sc).all()
    # rescore: -1 and out-of-range ids are no candidates, a repeat counts twice, k may exceed n_cand
    ids, sc = tref.rescore_expected(S[:1], np.array([[5, -1, 0, 5, 99, 3, 2]]), 6)
    assert ids.tolist() == [[2, 5, 5, 0, -1, -1]] and sc[0, :4].tolist() == [3.0, 3.0, 3.0, 1.0]
    a = (np.array([[1, 2]], np.int32), np.array([[0.0, 1.5]], np.float32))
    assert tref.same_result(a, (a[0], np.array([[-0.0, 1.5]], np.float32)))
    assert not tref.same_result(a, (a[0], np.array([[0.0, np.nextafter(np.float32(1.5), np.float32(2))]], np.float32)))
    assert not tref.same_result(a, (np.array([[2, 1]], np.int32), a[1]))


def test_bert_search_names_the_new_flags_and_refuses_what_they_exclude(tmp_path):
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    first = r.stderr.splitlines()[0]
    for word in ("--token-index", "--late"):
        assert word in r.stderr
    # the usage line keeps every option it named
    for word in ("-m MODEL", "-f TEXTS", "[-k 3]", "[--f32 | --i8 | --b1]", "[--rescore N]", "[--lists N]", "[--nprobe P]", "[-t THREADS]", "[--save PATH]",
                 "[--load PATH]", "[--long [--window W] [--stride S]]", "--maxsim N", "--cross-model PATH --cross N", "[--token-index]"):
        assert word in first, word
    assert "--sparse [WIDTH]" in r.stderr and "--hybrid SPLADE" in r.stderr
    f = tmp_path / "lines.txt"
    f.write_text("a\nb\n")
    base = [EXE, "-m", "nonexistent.bin", "-f", str(f)]
    excluded = (["--long"], ["--sparse"], ["--hybrid", "x.bin"], ["--cross-model", "x.bin", "--cross", "5"], ["--save", "x"], ["--load", "x"])
    for flag, extra in (("--token-index", ["--maxsim", "5", "--token-index"]), ("--late", ["--late"])):
        for ex in excluded:
            r = subprocess.run(base + extra + ex, capture_output=True, text=True, timeout=60)
            assert r.returncode == 2 and flag in r.stderr, (flag, ex, r.stderr)
    r = subprocess.run(base + ["--token-index"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--token-index goes with --maxsim" in r.stderr
    r = subprocess.run(base + ["--late", "--maxsim", "5"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--late" in r.stderr
