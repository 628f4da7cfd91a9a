"""Host tests of the hybrid search over the postings (include/bert_hip.h "Hybrid search", "Over the postings"): the exported names and
the binding, the plan of every cell tests/test_gpu_hybrid_inverted.py runs — taken from the hooks the search itself calls, so that the
GPU file never claims a geometry it did not get —, and a model of the scan that reads the dense score from a wrong place in three ways,
each of which the fixtures of the GPU file tell from the right one.  No GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import pybert

import hybrid_inverted_cases as hic
import topk_order_reference as tor
from conftest import ROOT

NEW_SYMBOLS = ["bert_hip_dense_sparse_search_inverted", "bert_hip_dense_sparse_search_inverted_device", "bert_hip_dense_sparse_search_inverted_texts"]
SIBLINGS = {"hybrid_search_inverted": "hybrid_search", "hybrid_search_inverted_device": "hybrid_search_device", "hybrid_search_inverted_texts": "hybrid_search_texts"}
HOOKS = (pybert.test_hybrid_chunk, pybert.test_sparse_postings_geometry)


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    declared = set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", text))
    for path in (pybert.LIB_PATH, pybert.TEST_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout.split()
        for sym in NEW_SYMBOLS:
            assert sym in exported, (path, sym)
        # the closed sets of tests/test_hybrid_host.py and of the token index stay closed: no new name holds either word
        assert not any("hybrid" in s or "token_index" in s for s in exported if s.startswith("bert_hip_dense_sparse")), path
    L = pybert.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in pybert.BERT_HIP_H_SYMBOLS and hasattr(L, sym), sym
        assert "hybrid" not in sym and "token_index" not in sym
    # the argument lists are the row-major entries', word for word
    for new, old in zip(NEW_SYMBOLS, ("bert_hip_hybrid_search", "bert_hip_hybrid_search_device", "bert_hip_hybrid_search_texts")):
        args = lambda name: re.sub(r"\s+", " ", re.search(r"BERT_API int32_t " + name + r"\(([^;]*)\);", text).group(1))
        assert args(new) == args(old), new
        assert getattr(L, new).argtypes == getattr(L, old).argtypes and getattr(L, new).restype == C.c_int32, new
    assert L.bert_hip_dense_sparse_search_inverted.argtypes[7:9] == [C.c_float, C.c_float]


def test_the_header_no_longer_lists_it_as_not_covered():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    assert "hybrid search over postings" not in text and "Over the postings" in text
    for path in ("include/bert_hip.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        t = open(os.path.join(ROOT, path)).read()
        assert not re.search(r"(Not covered|Out of scope)[^.]*[Ii]nverted", t), path
        assert not re.search(r"(Not covered|Out of scope|not covered)[^.]*hybrid search over (the )?postings", t), path
        assert "bert_hip_dense_sparse_search_inverted" in t, path


def test_the_binding_has_the_siblings_signatures_and_defaults():
    for new, old in SIBLINGS.items():
        a, b = inspect.signature(getattr(pybert.BertIndex, new)), inspect.signature(getattr(pybert.BertIndex, old))
        assert list(a.parameters) == list(b.parameters), new
        assert [p.default for p in a.parameters.values()] == [p.default for p in b.parameters.values()], new


def test_entry_points_return_minus_one_without_an_index(capfd):
    L = pybert.lib()
    out_i, out_s = np.full(4, 7, np.int32), np.full(4, 7.0, np.float32)
    capfd.readouterr()
    assert L.bert_hip_dense_sparse_search_inverted(None, None, 1, None, 1, None, None, 1.0, 1.0, None, 0, 4, out_i.ctypes.data, out_s.ctypes.data) == -1
    assert L.bert_hip_dense_sparse_search_inverted_device(None, None, 1, None, 1, None, None, 1.0, 1.0, None, 0, 4, out_i.ctypes.data, out_s.ctypes.data, None) == -1
    assert L.bert_hip_dense_sparse_search_inverted_texts(None, None, 1, 1, None, 4, 1.0, 1.0, 4, out_i.ctypes.data, out_s.ctypes.data) == -1
    err = capfd.readouterr().err
    assert err.count("no embedding index") == 3 and all(s in err for s in NEW_SYMBOLS)
    assert (out_i == 7).all() and (out_s == 7.0).all()


# ------------------------------------------------------------------------------------------------
# the plan of every GPU cell
# ------------------------------------------------------------------------------------------------
def test_the_random_cells_reach_three_segments_a_ragged_tail_and_a_second_chunk():
    for sd in hic.SPARSE:
        for seg in hic.R_SEGS:
            for nq in hic.R_NQS:
                for k in hic.R_KS:
                    hic.check_random_plan(hic.plan(*HOOKS, sd, hic.R_V, hic.R_ROWS, nq, k, seg), seg, nq)
    gone_d, gone_s, allow = hic.random_masks()
    assert len(np.intersect1d(gone_d, gone_s)) not in (0, len(gone_d))       # the two indexes' bitmaps differ and overlap
    for mode in hic.R_MODES:
        qual = hic.random_mode(mode)[3]
        assert (mode == "plain") == bool(qual.all())
        assert (10 < qual.sum() < 256) == (mode == "all three")                 # k = 256 there ends in -1 / -inf slots, elsewhere it is filled


def test_the_ordered_cells_walk_three_segments_and_end_a_slice_in_the_partial_one():
    for sd in hic.SPARSE:
        for k in hic.O_KS:
            for seg in hic.O_SEGS:
                for nq in hic.O_NQS[seg]:
                    hic.check_ordered_plan(hic.plan(*HOOKS, sd, tor.SPARSE_V, tor.SPARSE_ROWS, nq, k, seg), seg, nq)
    # one query of a tile is busy beside an idle one, first and last, in tiles of two
    fx = tor.hybrid_split_fixture("f32", "f32", 128, "plain", (1.0, 1.0))
    lay = tor.layouts(fx.kinds, fx.busy, fx.idle, hic.O_WALKED_NQ, 2)
    for b in fx.busy:
        first, last = lay[f"first:{b}"], lay[f"last:{b}"]
        assert all(first[q] == b and first[q + 1] in fx.idle for q in range(0, 608, 2)) and all(last[q + 1] == b and last[q] in fx.idle for q in range(0, 608, 2))


def test_the_many_slices_cells_are_seventeen_slices_and_three_chunks():
    for nq in hic.M_NQS:
        for k in hic.M_KS:
            hic.check_many_plan(hic.plan(*HOOKS, "f32", tor.SPARSE_V, tor.MANY_SPARSE_ROWS, nq, k, 0), nq)
    hic.check_many_plan(hic.plan(*HOOKS, "f32", tor.SPARSE_V, tor.MANY_SPARSE_ROWS, hic.M_CHUNK_NQ, 10, 0, pref=hic.M_CHUNK), hic.M_CHUNK_NQ, hic.M_CHUNK)


# ------------------------------------------------------------------------------------------------
# the fixtures can tell a wrong read of the score matrix
# ------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def test_the_fixtures_tell_each_wrong_read_of_the_dense_scores():
    right, in_seg, in_slice, call_q = hic.READS
    # many segments, one query each kind: a row's column inside its segment or slice is another row's score
    fx = tor.many_hybrid_fixture()
    lay = tor.many_layout(3)
    D, S = np.stack([fx.dsc[kk] for kk in lay]), np.stack([fx.ssc[kk] for kk in lay])
    qual = np.ones(fx.n, bool)
    for k in hic.M_KS:
        want = tor.of_layout(tor.hybrid_reference(fx, k), lay)
        p = hic.plan(*HOOKS, "f32", tor.SPARSE_V, fx.n, 3, k, 0)
        assert not _differs(hic.model_search(D, S, qual, 1.0, 1.0, k, p, right), want)
        for read in (in_seg, in_slice):
            got = hic.model_search(D, S, qual, 1.0, 1.0, k, p, read)
            busy = [i for i, kk in enumerate(lay) if kk != "const"]
            assert all(_differs((got[0][i:i + 1], got[1][i:i + 1]), (want[0][i:i + 1], want[1][i:i + 1])) for i in busy), (read, k)
    # slices of three segments (the ordered fixture, 609 queries): the row inside the slice is neither the global row nor the row inside the segment
    fo = tor.hybrid_split_fixture("f32", "f32", 128, "plain", (1.0, 1.0))
    olay = tor.layouts(fo.kinds, fo.busy, fo.idle, hic.O_WALKED_NQ, 2)["mixed"]
    Do, So = np.stack([fo.dsc[kk] for kk in olay]), np.stack([fo.ssc[kk] for kk in olay])
    po = hic.plan(*HOOKS, "f32", tor.SPARSE_V, fo.n, hic.O_WALKED_NQ, 128, 256)
    owant = tor.of_layout(tor.hybrid_reference(fo, 128, np.ones(fo.n, bool)), olay)
    results = {read: hic.model_search(Do, So, np.ones(fo.n, bool), 1.0, 1.0, 128, po, read) for read in (right, in_seg, in_slice)}
    assert not _differs(results[right], owant)
    assert _differs(results[in_seg], owant) and _differs(results[in_slice], owant) and _differs(results[in_seg], results[in_slice])
    # chunks of two: the query's index in the call is its index in the chunk in the first chunk alone
    lay5 = tor.many_layout(hic.M_CHUNK_NQ)
    D5, S5 = np.stack([fx.dsc[kk] for kk in lay5]), np.stack([fx.ssc[kk] for kk in lay5])
    want5 = tor.of_layout(tor.hybrid_reference(fx, 10), lay5)
    p5 = hic.plan(*HOOKS, "f32", tor.SPARSE_V, fx.n, hic.M_CHUNK_NQ, 10, 0, pref=hic.M_CHUNK)
    assert not _differs(hic.model_search(D5, S5, qual, 1.0, 1.0, 10, p5, right), want5)
    wrong = hic.model_search(D5, S5, qual, 1.0, 1.0, 10, p5, call_q)
    assert not _differs((wrong[0][:2], wrong[1][:2]), (want5[0][:2], want5[1][:2])) and _differs((wrong[0][2:], wrong[1][2:]), (want5[0][2:], want5[1][2:]))
    # unchunked, that wrong read is the right one: only the chunked cell can tell
    p1 = hic.plan(*HOOKS, "f32", tor.SPARSE_V, fx.n, hic.M_CHUNK_NQ, 10, 0)
    assert not _differs(hic.model_search(D5, S5, qual, 1.0, 1.0, 10, p1, call_q), want5)
