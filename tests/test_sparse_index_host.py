"""CPU-side tests of the sparse index (bert_hip.h "Sparse index"): the reference (tests/sparse_index_reference.py) against hand-computed
cases, the new symbols, the plan of the scan through its test hook, and the refusals that need no device."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from bert_cpp_amd import pybert as libbert

import sparse_index_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bert_hip_sparse_index_create", "bert_hip_sparse_index_free", "bert_hip_sparse_index_size", "bert_hip_sparse_index_reserve",
               "bert_hip_sparse_index_add", "bert_hip_sparse_index_add_device", "bert_hip_sparse_index_add_texts", "bert_hip_sparse_index_search",
               "bert_hip_sparse_index_search_device", "bert_hip_sparse_index_search_texts", "bert_hip_sparse_index_get_rows"]
HOOK = "bert_hip_test_sparse_scan_geometry"
f32 = np.float32


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def test_round_f32_hand_cases():
    assert ref.round_f32(Fraction(1)) == f32(1) and ref.round_f32(Fraction(-3, 2)) == f32(-1.5)
    ulp = Fraction(1, 2 ** 23)
    # ties go to the even mantissa, anything beyond a tie to the nearer value
    assert ref.round_f32(1 + ulp / 2) == f32(1)
    assert ref.round_f32(1 + ulp + ulp / 2) == f32(1 + 2 ** -22)
    assert ref.round_f32(1 + ulp / 2 + Fraction(1, 2 ** 80)) == f32(1 + 2 ** -23)
    assert ref.round_f32(1 + ulp + ulp / 2 - Fraction(1, 2 ** 80)) == f32(1 + 2 ** -23)
    # subnormals are spaced 2^-149; overflow is infinity
    assert ref.round_f32(Fraction(3, 2 ** 150)) == f32(2 ** -148) and ref.round_f32(Fraction(1, 2 ** 150)) == f32(0)
    assert ref.round_f32(Fraction(2) ** 128) == f32(np.inf) and ref.round_f32(-Fraction(2) ** 128) == f32(-np.inf)
    # (the largest f32 is 2^128 - 2^104; half a spacing above it is a tie that IEEE rounds to infinity, anything below stays finite)
    assert ref.round_f32(Fraction(2) ** 128 - Fraction(2) ** 103) == f32(np.inf)
    assert ref.round_f32(Fraction(2) ** 128 - Fraction(2) ** 103 - 1) == f32(np.finfo(np.float32).max)


def test_fma_is_rounded_once_where_a_float64_sum_rounds_twice():
    """w q = 2^-24 - 2^-70 exactly; acc = 1 + 2^-23 has an odd mantissa.  The exact sum lies just BELOW the half-way point
    1 + 2^-23 + 2^-24, so one rounding gives acc back.  A float64 sum rounds onto the half-way point first (2^-70 is below its
    resolution) and the second rounding, a tie, goes to the even neighbour 1 + 2^-22."""
    w, q, acc = f32(2 ** -12 * (1 + 2 ** -23)), f32(2 ** -12 * (1 - 2 ** -23)), f32(1 + 2 ** -23)
    assert Fraction(float(w)) * Fraction(float(q)) == Fraction(1, 2 ** 24) - Fraction(1, 2 ** 70)
    twice = f32(np.float64(w) * np.float64(q) + np.float64(acc))
    assert twice == f32(1 + 2 ** -22)
    assert ref.fma_f32(w, q, acc) == acc
    # the array form takes the exact route for this element, and the scalar chain agrees
    got = ref._fma_f32_array(np.array([w, f32(2)]), np.array([q, f32(3)]), np.array([acc, f32(1)]))
    assert got.tolist() == [float(acc), 7.0]
    assert ref.score([5, 9, -1], [f32(1), w, f32(0)], [9, 5], [q, acc]) == acc


def test_fma_zero_signs_and_underflow():
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32).item()
    assert bits(ref.fma_f32(-1.0, 0.0, 0.0)) == 0                       # -0 + +0
    assert bits(ref.fma_f32(3.0, -2.0, 6.0)) == 0                       # an exact cancellation
    assert bits(ref.fma_f32(-1e-30, 1e-30, 0.0)) == 0x80000000          # a non-zero result that underflows keeps its sign
    assert bits(ref.fma_f32(-1.0, 0.0, -0.0)) == 0x80000000
    assert ref.fma_f32(2 ** -100, 2 ** -49, 0.0) == f32(2 ** -149) and ref.fma_f32(2 ** -100, 2 ** -50, 0.0) == f32(0)


def test_array_scores_equal_the_scalar_chain():
    """scores() (float64 where that is provably one rounding) against the all-rational scalar chain, on operands of very different
    magnitudes so that most float64 sums are inexact."""
    rng = np.random.default_rng(5)
    V, width, n, nq, kq = 50, 24, 40, 6, 30
    ids = np.full((n, width), -1, np.int32)
    w = np.zeros((n, width), np.float32)
    for r in range(n):
        c = int(rng.integers(0, width + 1))
        ids[r, :c] = rng.choice(V, c, replace=False)
        w[r, :c] = (rng.standard_normal(c) * 10.0 ** rng.integers(-6, 7, c)).astype(np.float32)
    st_i, st_w = ref.stored_rows(ids, w, width, "f32")
    q_ids = np.stack([rng.permutation(V)[:kq] for _ in range(nq)]).astype(np.int32)
    q_ids[0, ::3] = -1
    q_w = (rng.standard_normal((nq, kq)) * 10.0 ** rng.integers(-6, 7, (nq, kq))).astype(np.float32)
    got = ref.scores(st_i, st_w, q_ids, q_w, V)
    for qi in range(nq):
        for r in range(n):
            assert got[qi, r].view(np.uint32) == np.asarray(ref.score(st_i[r], st_w[r], q_ids[qi], q_w[qi])).view(np.uint32), (qi, r)


def test_order_rule():
    s = np.array([1.0, np.nan, 3.0, 3.0, -0.0, 0.0, -np.inf, 3.0], np.float32)
    ids, sc = ref.topk(s, 10)
    assert ids.tolist() == [2, 3, 7, 0, 4, 5, 6, -1, -1, -1]             # equal scores (== : +0 and -0 too) by id, NaN never
    assert sc[:7].tolist() == [3.0, 3.0, 3.0, 1.0, 0.0, 0.0, -np.inf] and np.all(np.isneginf(sc[7:]))
    assert np.signbit(sc[4]) and not np.signbit(sc[5])                   # the scores come back as they are
    assert ref.topk(s, 2)[0].tolist() == [2, 3]
    assert ref.topk(np.zeros(0, np.float32), 2)[0].tolist() == [-1, -1]


def test_stored_rows_sort_drop_and_round():
    # f16 has 11 significant bits: at 2048 the spacing is 2.  2049 is a tie (down to even 2048), 2051 a tie (up to even 2052),
    # 2049.5 rounds up, 2050.9 rounds down; 1e-8 underflows to +0 and is still a term
    ids = np.array([[7, -1, 3, 9, 1, -1, 4], [-1] * 7], np.int32)
    w = np.array([[2049.0, 99.0, 2051.0, 2049.5, 2050.9, 99.0, 1e-8], [5.0] * 7], np.float32)
    si, sw = ref.stored_rows(ids, w, 8, "f16")
    assert si.tolist() == [[1, 3, 4, 7, 9, -1, -1, -1], [-1] * 8]
    assert sw[0].tolist() == [2050.0, 2052.0, 0.0, 2048.0, 2050.0, 0.0, 0.0, 0.0] and not sw[1].any()
    si, sw = ref.stored_rows(ids, w, 8, "f32")
    assert sw[0, :5].tolist() == [w[0, 4], 2051.0, w[0, 6], 2049.0, 2049.5]
    # a search over them: row 0 matches ids 3 and 9, row 1 nothing (+0, and it still competes)
    ri, rs = ref.search(si, sw, np.array([[9, 3, 2]], np.int32), np.array([[2.0, -1.0, 5.0]], np.float32), 16, 3)
    assert ri.tolist() == [[0, 1, -1]] and rs[0, :2].tolist() == [2 * 2049.5 - 2051.0, 0.0]


# ------------------------------------------------------------------------------------------------
# symbols
# ------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "bert_hip.h")).read()
    declared = set(re.findall(r"BERT_API[^;(]*?\b(bert_\w+)\s*\(", text))
    L, T = libbert.lib(), libbert.test_lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in libbert.BERT_HIP_H_SYMBOLS, sym
        assert hasattr(L, sym) and hasattr(T, sym), sym
    assert "struct bert_hip_sparse_index;" in text
    test_text = open(os.path.join(ROOT, "include", "bert_hip_test.h")).read()
    assert HOOK in test_text and HOOK in libbert.BERT_HIP_TEST_H_SYMBOLS
    assert hasattr(T, HOOK) and not hasattr(L, HOOK)


# ------------------------------------------------------------------------------------------------
# the plan of the scan
# ------------------------------------------------------------------------------------------------
def _image_bytes(V):
    words = (V + 31) // 32
    return (words * 4 + (words * 2 + 3) // 4 * 4 + 256 * 4 + 15) // 16 * 16


@pytest.mark.parametrize("args, want", [
    # (dtype, n_vocab, n_rows, nq, k)
    ((0, 30522, 0, 1, 10), dict(qb=1, n_qtiles=1, n_slices=1, slice_rows=256, L=512)),
    ((0, 30522, 1000, 70, 10), dict(qb=2, n_qtiles=35, n_slices=1, slice_rows=1024, L=512)),
    ((0, 30522, 5000, 9, 10), dict(qb=2, n_qtiles=5, n_slices=2, slice_rows=2560, L=512)),
    ((1, 65536, 5000, 1, 256), dict(qb=1, n_qtiles=1, n_slices=2, slice_rows=2560, L=1024)),
    ((0, 262144, 130, 70, 10), dict(qb=2, n_qtiles=35, n_slices=1, slice_rows=256, L=512)),
    ((0, 262144, 130, 70, 256), dict(qb=2, n_qtiles=35, n_slices=1, slice_rows=256, L=1024)),
    ((0, 30522, 1000000, 1, 10), dict(qb=1, n_qtiles=1, n_slices=435, slice_rows=2304, L=512)),
    ((1, 30522, 1000000, 4096, 100), dict(qb=2, n_qtiles=2048, n_slices=1, slice_rows=1000192, L=512)),
])
def test_scan_geometry_table(args, want):
    got = libbert.test_sparse_scan_geometry(*args)
    per_query = _image_bytes(args[1]) + want["L"] * 8 + 4
    assert got == dict(want, lds=want["qb"] * per_query)


def test_scan_geometry_invariants():
    for dtype in (0, 1):
        for V in (1, 31, 32, 33, 40, 1000, 30522, 65535, 65536, 65537, 100000, 262143, 262144):
            if dtype == 1 and V > 65536:
                assert libbert.test_sparse_scan_geometry(dtype, V, 100, 1, 1) is None
                continue
            for k in (1, 128, 129, 256):
                for nq in (1, 2, 3, 70, 4096):
                    for n_rows in (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 4095, 4096, 4097, 5000, 1000000, 2 ** 31 - 65):
                        g = libbert.test_sparse_scan_geometry(dtype, V, n_rows, nq, k)
                        assert g is not None and g["qb"] >= 1, (dtype, V, n_rows, nq, k)
                        assert g["lds"] <= 160 * 1024 and g["lds"] == g["qb"] * (_image_bytes(V) + g["L"] * 8 + 4)
                        assert g["n_qtiles"] == -(-nq // g["qb"]) and g["qb"] <= nq
                        # every row in exactly one slice; slices start at whole blocks (and whole steps of four waves); no slice is empty
                        assert g["slice_rows"] % 256 == 0 and g["slice_rows"] % 64 == 0 and g["n_slices"] >= 1
                        assert g["n_slices"] * g["slice_rows"] >= n_rows > (g["n_slices"] - 1) * g["slice_rows"] - (n_rows == 0)
                        # a queue takes a whole step's rows behind the top-k
                        assert g["L"] - k - 256 >= 0 and g["L"] & (g["L"] - 1) == 0


def test_scan_geometry_refusals():
    G = libbert.test_sparse_scan_geometry
    assert G(2, 100, 10, 1, 1) is None and G(-1, 100, 10, 1, 1) is None
    assert G(0, 0, 10, 1, 1) is None and G(0, 262145, 10, 1, 1) is None and G(1, 65537, 10, 1, 1) is None
    assert G(0, 100, -1, 1, 1) is None and G(0, 100, 10, 0, 1) is None
    assert G(0, 100, 10, 1, 0) is None and G(0, 100, 10, 1, 257) is None
    assert libbert.test_lib().bert_hip_test_sparse_scan_geometry(0, 100, 10, 1, 1, None) == -1


# ------------------------------------------------------------------------------------------------
# refusals that need no device
# ------------------------------------------------------------------------------------------------
def test_null_index_and_null_context(capfd):
    L = libbert.lib()
    ids = np.full((1, 4), 7, np.int32)
    w = np.full((1, 4), 7.0, np.float32)
    p = lambda a: a.ctypes.data
    assert not L.bert_hip_sparse_index_create(None, 0, 128, 0)
    assert "no context" in capfd.readouterr().err
    assert L.bert_hip_sparse_index_size(None) == -1
    L.bert_hip_sparse_index_free(None)
    txt = (C.c_char_p * 1)(b"a")
    assert L.bert_hip_sparse_index_reserve(None, 1, 1, 1) == -1
    assert L.bert_hip_sparse_index_add(None, 1, 4, p(ids), p(w)) == -1
    assert L.bert_hip_sparse_index_add_device(None, 1, 4, None, None, None) == -1
    assert L.bert_hip_sparse_index_add_texts(None, 1, 1, txt) == -1
    assert L.bert_hip_sparse_index_search(None, 1, 4, p(ids), p(w), 4, p(ids), p(w)) == -1
    assert L.bert_hip_sparse_index_search_device(None, 1, 4, None, None, 4, None, None, None) == -1
    assert L.bert_hip_sparse_index_search_texts(None, 1, 1, txt, 4, 4, p(ids), p(w)) == -1
    assert L.bert_hip_sparse_index_get_rows(None, 1, p(ids), p(ids), p(w)) == -1
    assert capfd.readouterr().err.count("no index") == 8
    assert (ids == 7).all() and (w == 7.0).all()


def test_tokenizer_only_context_has_no_sparse_index(sparse_vocab_model, capfd):
    m = libbert.BertModel(sparse_vocab_model, tokenizer_only=True)
    assert not m.lib.bert_hip_sparse_index_create(m.ctx, 0, 128, 0)
    assert "tokenizer-only" in capfd.readouterr().err
    with pytest.raises(RuntimeError):
        m.sparse_index()
    with pytest.raises(ValueError):
        m.sparse_index(dtype="i8")
    m.close()
