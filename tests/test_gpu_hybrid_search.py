"""GPU tests of the hybrid search (include/bert_hip.h "Hybrid search"): the exact top-k of H = (w_dense * D) + (w_sparse * S) over the
rows live in an embedding index, live in a sparse index and allowed.  The reference of a result is tests/hybrid_reference.py: S from
sparse_index_reference.scores over the stored rows, D from index_reference.exact_scores (i8, b1) or, for f32 / f16 — whose MFMA chain
is not restated in Python —, read through the dense index's public rescore (every row a candidate, 256 at a time); the rows that do not
qualify set to NaN, combine, topk.  Equality means bits, in ids and in scores."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import hip_graph
import hybrid_reference as href
import index_reference as iref
import sparse_index_reference as sref
import test_gpu_sparse_index_lifecycle as lc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
OK = hip_graph.HIP_SUCCESS
DENSE = ["f32", "f16", "i8", "b1"]
SPARSE = ["f32", "f16"]
_same = lc._same


def _p(a):
    return a.ctypes.data


@pytest.fixture(scope="module")
def model(make_model):
    """any model: both indexes only need the context's device"""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hip():
    return hip_graph.Hip()


@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    dim: int
    width: int
    V: int
    ties: bool
    nq: int
    kq: int


CASES = {
    "n 1": Case(1, 20, 4, 64, True, 3, 16),
    "n 65, dim 384, width 256, V 30522, 33 queries": Case(65, 384, 256, 30522, False, 33, 64),
    "n 300, dim 20, width 4, V 64: ties, 65 queries": Case(300, 20, 4, 64, True, 65, 16),
    "n 300, dim 384, width 256, V 30522": Case(300, 384, 256, 30522, False, 3, 64),
    "n 4200, dim 20: two slices, 33 queries": Case(4200, 20, 4, 64, True, 33, 16),
}
N300 = "n 300, dim 20, width 4, V 64: ties, 65 queries"
N4200 = "n 4200, dim 20: two slices, 33 queries"
_DATA, _S, _D = {}, {}, {}


def _data(name):
    """dense rows and queries (unit f32), sparse rows and queries of a case, made once"""
    if name not in _DATA:
        c = CASES[name]
        rng = np.random.default_rng(len(name) + c.n)
        rows = iref.unit(rng.standard_normal((c.n, c.dim)))
        queries = iref.unit(rng.standard_normal((c.nq, c.dim)))
        ids, w = lc._terms(rng, c.n, c.width, c.V, c.width, c.ties)
        q_ids, q_w = lc._terms(rng, c.nq, c.kq, c.V, c.kq, c.ties)
        for a in (rows, queries, ids, w, q_ids, q_w):
            a.setflags(write=False)
        _DATA[name] = (rows, queries, ids, w, q_ids, q_w)
    return _DATA[name]


def _sparse_scores(name, sd):
    """S [nq][n]: the reference's scores over the stored rows, computed once"""
    if (name, sd) not in _S:
        c = CASES[name]
        rows, queries, ids, w, q_ids, q_w = _data(name)
        st = sref.stored_rows(ids, w, c.width, sd)
        _S[(name, sd)] = sref.scores(st[0], st[1], q_ids, q_w, c.V)
        _S[(name, sd)].setflags(write=False)
    return _S[(name, sd)]


def _rescored(dix, queries, n):
    """D [nq][n] through the public rescore: all rows as candidates in chunks of 256 with k = 256 (a row the index skips stays NaN)"""
    nq = len(queries)
    D = np.full((nq, n), np.nan, np.float32)
    for c0 in range(0, n, 256):
        m = min(256, n - c0)
        cand = np.full((nq, 256), -1, np.int32)
        cand[:, :m] = np.arange(c0, c0 + m)
        ids, sc = dix.rescore(queries, cand, 256)
        for q in range(nq):
            ok = ids[q] >= 0
            D[q, ids[q][ok]] = sc[q][ok]
    return D


def _dense_scores(model, name, dd):
    """D [nq][n] of the full index, computed once"""
    if (name, dd) not in _D:
        c = CASES[name]
        rows, queries = _data(name)[:2]
        if dd in ("i8", "b1"):
            D = iref.exact_scores(queries, rows, dd)
        else:
            ix = model.index(c.dim, dd)
            ix.add(rows)
            D = _rescored(ix, queries, c.n)
            ix.close()
            assert not np.isnan(D).any()
        D.setflags(write=False)
        _D[(name, dd)] = D
    return _D[(name, dd)]


def _pair(model, name, dd, sd, sparse_model=None):
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    dix = model.index(c.dim, dd)
    six = (sparse_model or model).sparse_index(c.width, sd, n_vocab=c.V)
    assert dix.add(rows) == 0 and six.add(ids, w) == 0
    return dix, six


def _want(model, name, dd, sd, qual, wd, ws, k, q=slice(None)):
    c = CASES[name]
    qual = np.ones(c.n, bool) if qual is None else qual
    return href.search(_dense_scores(model, name, dd)[q], _sparse_scores(name, sd)[q], qual, wd, ws, k)


def _raw(model, dix, six, queries, q_ids, q_w, wd, ws, words, n_words, k, out_i, out_s, kq=None):
    q, qi, qw = np.ascontiguousarray(queries, np.float32), np.ascontiguousarray(q_ids, np.int32), np.ascontiguousarray(q_w, np.float32)
    return model.lib.bert_hip_hybrid_search(dix.ix, six.ix, len(q), _p(q), qi.shape[1] if kq is None else kq, _p(qi), _p(qw), wd, ws,
                                            None if words is None else _p(words), n_words, k, _p(out_i), _p(out_s))


# ------------------------------------------------------------------------------------------------
# 1. shapes against the reference
# ------------------------------------------------------------------------------------------------
SHAPES = [(N300, dd, sd) for dd in DENSE for sd in SPARSE] + \
         [(name, dd, sd) for name in CASES if name != N300 for dd, sd in (("f16", "f32"), ("b1", "f16"))]


@pytest.mark.parametrize("name, dd, sd", SHAPES)
def test_shapes_equal_the_reference(model, name, dd, sd):
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    if name == N4200:
        g = pybert.test_sparse_scan_geometry(SPARSE.index(sd), c.V, c.n, c.nq, 10)
        assert g["n_slices"] == 2 and c.n % g["slice_rows"] != 0, g
    if c.nq == 33:
        assert pybert.test_hybrid_chunk(c.n, c.nq) == (32, (c.n + 63) // 64 * 64)          # a second chunk of one query
    dix, six = _pair(model, name, dd, sd)
    for k in (1, 10, 256):
        want = _want(model, name, dd, sd, None, 1.0, 1.0, k)
        if k > c.n:
            assert (want[0][:, c.n:] == -1).all() and np.isneginf(want[1][:, c.n:]).all()
        assert _same(dix.hybrid_search(six, queries, q_ids, q_w, k), want), k
    assert _same(dix.hybrid_search(six, queries, q_ids, q_w, 10, 0.7, 0.3), _want(model, name, dd, sd, None, 0.7, 0.3, 10))
    if c.ties and c.n >= 300:
        # tied sparse weights alone: few distinct scores, the order rule decides almost every slot
        assert max(len(np.unique(s)) for s in _sparse_scores(name, sd)) < c.n // 4
        assert _same(dix.hybrid_search(six, queries, q_ids, q_w, 256, 0.0, 1.0), _want(model, name, dd, sd, None, 0.0, 1.0, 256))
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 2. weights
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dd, sd", [("f16", "f32"), ("b1", "f16"), ("i8", "f32"), ("f32", "f16")])
def test_weights(model, dd, sd, capfd):
    name = N300
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    dix, six = _pair(model, name, dd, sd)
    k = 20
    # (1, 0) and (0, 1): the two plain searches, ids equal and scores numerically equal (the sign of a zero may differ)
    got = dix.hybrid_search(six, queries, q_ids, q_w, k, 1.0, 0.0)
    plain = dix.search(queries, k)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    got = dix.hybrid_search(six, queries, q_ids, q_w, k, 0.0, 1.0)
    plain = six.search(q_ids, q_w, k)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    for wd, ws in ((0.7, 0.3), (1.0, 1e-3), (-1.0, 1.0), (0.0, 0.0)):
        got = dix.hybrid_search(six, queries, q_ids, q_w, k, wd, ws)
        assert _same(got, _want(model, name, dd, sd, None, wd, ws, k)), (wd, ws)
        if (wd, ws) == (0.0, 0.0) and dd != "i8":
            # (the tied sparse weights are positive: every score is +0, and the smallest ids win)
            assert (got[0] == np.arange(k)).all() and (got[1] == 0).all() and not np.signbit(got[1]).any()
    # weights that are not finite are refused, outputs untouched
    out_i, out_s = np.full((c.nq, k), 7, np.int32), np.full((c.nq, k), 7.0, np.float32)
    capfd.readouterr()
    for wd, ws in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf)):
        assert _raw(model, dix, six, queries, q_ids, q_w, wd, ws, None, 0, k, out_i, out_s) == -2
        assert "finite" in capfd.readouterr().err
        with pytest.raises(ValueError):
            dix.hybrid_search(six, queries, q_ids, q_w, k, wd, ws)
    assert (out_i == 7).all() and (out_s == 7.0).all()
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 3. masks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, dd, sd", [(N300, "f16", "f32"), (N300, "b1", "f16"), (N4200, "f16", "f32"), (N4200, "i8", "f16")])
def test_allow_lists_equal_the_reference(model, name, dd, sd):
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    nq = min(c.nq, 9)
    q = (queries[:nq], q_ids[:nq], q_w[:nq])
    dix, six = _pair(model, name, dd, sd)
    plain = dix.hybrid_search(six, *q, 10)
    pats = lc._patterns(c.n)
    assert len(pats) == 8
    for pname, qual in pats.items():
        for k in (10, 256):
            want = _want(model, name, dd, sd, qual, 1.0, 0.5, k, slice(0, nq))
            if qual.sum() < k:
                assert (want[0][:, qual.sum():] == -1).all() and np.isneginf(want[1][:, qual.sum():]).all()
            assert _same(dix.hybrid_search(six, *q, k, 1.0, 0.5, allow=qual), want), (pname, k)
        # words beyond ceil(size / 32) and bits at and beyond size are the caller's: all ones here
        assert _same(dix.hybrid_search(six, *q, 10, 1.0, 0.5, allow=lc._poisoned_words(qual)), _want(model, name, dd, sd, qual, 1.0, 0.5, 10, slice(0, nq))), pname
        if pname == "all ones":
            assert _same(dix.hybrid_search(six, *q, 10, allow=qual), plain)
    dix.close()
    six.close()


@pytest.mark.parametrize("where", ["dense", "sparse", "both"])
@pytest.mark.parametrize("name, dd, sd", [(N300, "f16", "f32"), (N300, "i8", "f16"), (N4200, "b1", "f32")])
def test_rows_removed_in_either_index_never_come_back(model, name, dd, sd, where):
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    nq = min(c.nq, 9)
    q = (queries[:nq], q_ids[:nq], q_w[:nq])
    pats = lc._patterns(c.n, seed=1)
    a, b, allow = pats["random 50 %"], pats["a block cleared between two full ones"] & (np.arange(c.n) % 3 != 0), pats["alternating"]
    dix, six = _pair(model, name, dd, sd)
    live = np.ones(c.n, bool)
    if where in ("dense", "both"):
        assert dix.remove(np.flatnonzero(~a).astype(np.int32)) == (~a).sum()
        live &= a
    if where in ("sparse", "both"):
        assert six.remove(np.flatnonzero(~b).astype(np.int32)) == (~b).sum()
        live &= b
    for k in (10, 256):
        assert _same(dix.hybrid_search(six, *q, k), _want(model, name, dd, sd, live, 1.0, 1.0, k, slice(0, nq))), k
        assert _same(dix.hybrid_search(six, *q, k, allow=lc._poisoned_words(allow)), _want(model, name, dd, sd, live & allow, 1.0, 1.0, k, slice(0, nq))), k
    # rows added after the removals are live in both
    extra = iref.unit(np.random.default_rng(2).standard_normal((3, c.dim)))
    assert dix.add(extra) == c.n and six.add(ids[:3], w[:3]) == c.n
    got = dix.hybrid_search(six, extra, ids[:3, :min(c.width, 16)], w[:3, :min(c.width, 16)], 5, 1.0, 0.0)
    assert (got[0][:, 0] == c.n + np.arange(3)).all()
    dix.close()
    six.close()


def test_too_few_allow_words_and_an_inf_row(model, hip, capfd):
    name = N300
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    bad = np.array(rows)
    bad[5, 3] = np.inf
    dix = model.index(c.dim, "i8")
    six = model.sparse_index(c.width, "f32", n_vocab=c.V)
    dix.add(bad)
    six.add(ids, w)
    # an i8 row that held an inf has D = NaN, hence H = NaN: never returned, with any weights
    D = iref.exact_scores(queries, bad, "i8")
    assert np.isnan(D[:, 5]).all() and not np.isnan(np.delete(D, 5, axis=1)).any()
    for wd, ws in ((1.0, 1.0), (0.0, 1.0)):
        got = dix.hybrid_search(six, queries, q_ids, q_w, 256, wd, ws, allow=np.arange(c.n) < 256)
        assert _same(got, href.search(D, _sparse_scores(name, "f32"), np.arange(c.n) < 256, wd, ws, 256))
        assert not (got[0] == 5).any() and (got[0][:, 254] >= 0).all() and (got[0][:, 255] == -1).all()
    # n_words < ceil(size / 32) is refused by the host and the device form, outputs untouched
    words = np.full(10, 0xFFFFFFFF, np.uint32)
    out_i, out_s = np.full((c.nq, 4), 7, np.int32), np.full((c.nq, 4), 7.0, np.float32)
    capfd.readouterr()
    assert _raw(model, dix, six, queries, q_ids, q_w, 1.0, 1.0, words, 9, 4, out_i, out_s) == -2
    assert "allow-list" in capfd.readouterr().err
    d = [hip.upload(np.array(a)) for a in (queries, q_ids, q_w, words)]
    d_i, d_s = hip.nans((c.nq, 4), np.int32), hip.nans((c.nq, 4))
    assert model.lib.bert_hip_hybrid_search_device(dix.ix, six.ix, c.nq, d[0], c.kq, d[1], d[2], 1.0, 1.0, d[3], 9, 4, d_i, d_s, None) == -2
    assert "allow-list" in capfd.readouterr().err
    assert (hip.download(d_i, (c.nq, 4), np.int32) == -1).all() and (out_i == 7).all() and (out_s == 7.0).all()
    # exactly the words needed are enough; allow == NULL ignores n_words
    assert model.lib.bert_hip_hybrid_search_device(dix.ix, six.ix, c.nq, d[0], c.kq, d[1], d[2], 1.0, 1.0, d[3], 10, 4, d_i, d_s, None) == 0
    assert _same((hip.download(d_i, (c.nq, 4), np.int32), hip.download(d_s, (c.nq, 4))), href.search(D, _sparse_scores(name, "f32"), np.ones(c.n, bool), 1.0, 1.0, 4))
    assert _raw(model, dix, six, queries, q_ids, q_w, 1.0, 1.0, None, 0, 4, out_i, out_s) == 0
    assert _same((out_i, out_s), href.search(D, _sparse_scores(name, "f32"), np.ones(c.n, bool), 1.0, 1.0, 4))
    hip.free(*d, d_i, d_s)
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 4. chunking, batch, k, entry point
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, dd, sd", [(N300, "f16", "f32"), (N300, "i8", "f16"), (N4200, "f32", "f16"), (N4200, "b1", "f32")])
def test_a_result_does_not_depend_on_chunking_batch_k_or_entry_point(model, hip, name, dd, sd):
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    rng = np.random.default_rng(5)
    # 65 queries at both sizes: the case's, repeated in another order
    pick = rng.permutation(np.resize(np.arange(c.nq), 65))
    Q, QI, QW = queries[pick], q_ids[pick], q_w[pick]
    dix, six = _pair(model, name, dd, sd)
    qual = lc._patterns(c.n)["random 50 %"]
    base = dix.hybrid_search(six, Q, QI, QW, 100, 0.6, 0.4)
    masked = dix.hybrid_search(six, Q, QI, QW, 100, 0.6, 0.4, allow=qual)
    assert _same(base, _want(model, name, dd, sd, None, 0.6, 0.4, 100, pick))
    assert _same(masked, _want(model, name, dd, sd, qual, 0.6, 0.4, 100, pick))
    try:
        for hc in (1, 3, 40):
            model.set_option("hybrid_chunk_queries", str(hc))
            assert _same(dix.hybrid_search(six, Q, QI, QW, 100, 0.6, 0.4), base), hc
            assert _same(dix.hybrid_search(six, Q, QI, QW, 100, 0.6, 0.4, allow=qual), masked), hc
    finally:
        model.set_option("hybrid_chunk_queries", "0")
    # a query alone is the same query inside the batch; top-10 is the prefix of top-100
    for pos in (0, 31, 32, 64):
        alone = dix.hybrid_search(six, Q[pos:pos + 1], QI[pos:pos + 1], QW[pos:pos + 1], 100, 0.6, 0.4)
        assert _same(alone, (base[0][pos:pos + 1], base[1][pos:pos + 1])), pos
    top10 = dix.hybrid_search(six, Q, QI, QW, 10, 0.6, 0.4)
    assert _same(top10, (base[0][:, :10], base[1][:, :10]))
    # the device entry point, plain and with a device allow-list
    words = pybert.allow_words(qual, c.n)
    d = [hip.upload(np.array(a)) for a in (Q, QI, QW, words)]
    d_i, d_s = hip.nans((65, 100), np.int32), hip.nans((65, 100))
    dix.hybrid_search_device(six, 65, d[0], c.kq, d[1], d[2], 100, d_i, d_s, 0.6, 0.4)
    assert _same((hip.download(d_i, (65, 100), np.int32), hip.download(d_s, (65, 100))), base)
    dix.hybrid_search_device(six, 65, d[0], c.kq, d[1], d[2], 100, d_i, d_s, 0.6, 0.4, 0, d[3], len(words))
    assert _same((hip.download(d_i, (65, 100), np.int32), hip.download(d_s, (65, 100))), masked)
    hip.free(*d, d_i, d_s)
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 5. build history
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dd, sd", [("f16", "f32"), ("i8", "f16"), ("b1", "f32"), ("f32", "f16")])
def test_a_result_does_not_depend_on_how_the_indexes_were_built(model, dd, sd):
    name = N4200
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    one = _pair(model, name, dd, sd)
    want = one[0].hybrid_search(one[1], queries, q_ids, q_w, 50, 0.5, 2.0)
    assert _same(want, _want(model, name, dd, sd, None, 0.5, 2.0, 50))
    # three adds that start and end inside blocks, grown storage
    dix, six = model.index(c.dim, dd), model.sparse_index(c.width, sd, n_vocab=c.V)
    for lo, hi in ((0, 70), (70, 1500), (1500, c.n)):
        assert dix.add(rows[lo:hi]) == lo and six.add(ids[lo:hi], w[lo:hi]) == lo
    assert _same(dix.hybrid_search(six, queries, q_ids, q_w, 50, 0.5, 2.0), want)
    # reserved storage and workspace, different add boundaries on the two sides
    rdix, rsix = model.index(c.dim, dd), model.sparse_index(c.width, sd, n_vocab=c.V)
    rdix.hybrid_reserve(rsix, 6000, c.nq, 50)
    rdix.add(rows[:4000])
    rdix.add(rows[4000:])
    rsix.add(ids[:100], w[:100])
    rsix.add(ids[100:], w[100:])
    assert _same(rdix.hybrid_search(rsix, queries, q_ids, q_w, 50, 0.5, 2.0), want)
    for x in (*one, dix, six, rdix, rsix):
        x.close()


# ------------------------------------------------------------------------------------------------
# 6. two contexts, refusals
# ------------------------------------------------------------------------------------------------
def test_two_contexts_and_refusals(model, make_model, capfd):
    name = N300
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    path, _ = make_model("tiny", "f16", 0)
    other = pybert.BertModel(path)
    assert other.ctx != model.ctx
    same = _pair(model, name, "f16", "f32")
    want = same[0].hybrid_search(same[1], queries, q_ids, q_w, 30, 0.7, 0.3)
    dix, six = _pair(model, name, "f16", "f32", sparse_model=other)
    assert _same(dix.hybrid_search(six, queries, q_ids, q_w, 30, 0.7, 0.3), want)
    try:
        # the tuning key is read from the SPARSE index's context
        other.set_option("hybrid_chunk_queries", "7")
        assert _same(dix.hybrid_search(six, queries, q_ids, q_w, 30, 0.7, 0.3), want)
    finally:
        other.set_option("hybrid_chunk_queries", "0")
    L = model.lib
    out_i, out_s = np.full((c.nq, 4), 7, np.int32), np.full((c.nq, 4), 7.0, np.float32)
    capfd.readouterr()

    def refused(r, what):
        err = capfd.readouterr().err
        assert r == -2 and what in err, (r, what, err)
        assert (out_i == 7).all() and (out_s == 7.0).all()

    for kq in (0, 257):
        refused(_raw(model, dix, six, queries, q_ids, q_w, 1.0, 1.0, None, 0, 4, out_i, out_s, kq=kq), "kq must be")
    for k in (0, 257):
        refused(_raw(model, dix, six, queries, q_ids, q_w, 1.0, 1.0, None, 0, k, out_i, out_s), "k must be")
        refused(L.bert_hip_hybrid_search_device(dix.ix, six.ix, 1, None, c.kq, None, None, 1.0, 1.0, None, 0, k, None, None, None), "k must be")
        refused(L.bert_hip_hybrid_reserve(dix.ix, six.ix, 10, 1, k), "reserve")
    q, qi, qw = np.array(queries), np.array(q_ids), np.array(q_w)
    refused(L.bert_hip_hybrid_search(dix.ix, six.ix, c.nq, None, c.kq, _p(qi), _p(qw), 1.0, 1.0, None, 0, 4, _p(out_i), _p(out_s)), "pointers")
    refused(L.bert_hip_hybrid_search(dix.ix, six.ix, -1, _p(q), c.kq, _p(qi), _p(qw), 1.0, 1.0, None, 0, 4, _p(out_i), _p(out_s)), "n_queries")
    # the host form checks the sparse queries as bert_hip_sparse_index_search does
    bad = qi.copy()
    bad[1, 0] = c.V
    refused(_raw(model, dix, six, q, bad, qw, 1.0, 1.0, None, 0, 4, out_i, out_s), "outside")
    badw = qw.copy()
    badw[0, int(np.flatnonzero(qi[0] >= 0)[0])] = np.nan                     # (entry 0 of _terms holds as many ids as fit)
    refused(_raw(model, dix, six, q, qi, badw, 1.0, 1.0, None, 0, 4, out_i, out_s), "not finite")
    # sizes that disagree
    assert six.add(ids[:1], w[:1]) == c.n
    refused(_raw(model, dix, six, queries, q_ids, q_w, 1.0, 1.0, None, 0, 4, out_i, out_s), "rows")
    with pytest.raises(ValueError):
        dix.hybrid_search(six, queries, q_ids, q_w, 4)
    # n_queries == 0 is a no-op; an empty pair is valid
    assert dix.add(rows[:1]) == c.n
    assert L.bert_hip_hybrid_search(dix.ix, six.ix, 0, None, c.kq, None, None, 1.0, 1.0, None, 0, 4, None, None) == 0
    e_d, e_s = model.index(c.dim, "i8"), other.sparse_index(c.width, "f16", n_vocab=c.V)
    got = e_d.hybrid_search(e_s, queries, q_ids, q_w, 3)
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    got = e_d.hybrid_search(e_s, queries, q_ids, q_w, 3, allow=np.zeros(0, np.uint32))
    assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    for x in (*same, dix, six, e_d, e_s):
        x.close()
    other.close()


# ------------------------------------------------------------------------------------------------
# 7. texts
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_model(model_dir, tok_golden):
    """tiny dims over the golden tokenizer's vocabulary, with the MLM head; the same without it"""
    n = tok_golden["n_vocab"]
    vocab = [f"[unused{i}]" for i in range(n)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    for i, p in tok_golden["sparse_vocab"].items():
        vocab[int(i)] = p
    hp = dataclasses.replace(gf.MODEL_DIMS["tiny"], n_vocab=n)
    paths = []
    for head in (True, False):
        path = os.path.join(model_dir, f"hybrid_text_{int(head)}.bin")
        gf.write_model(path, hp, gf.synthetic_weights(hp, 11, mlm_head=head), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
        paths.append(path)
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    return paths[0], paths[1], words


@pytest.mark.parametrize("dd, sd", [("f16", "f32"), ("i8", "f16")])
def test_text_route_is_encode_and_encode_sparse_fed_to_the_search(text_model, dd, sd, capfd):
    path, without, words = text_model
    m = pybert.BertModel(path)
    rng = np.random.default_rng(4)
    texts = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 40, size=70)]
    queries = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 12, size=9)]
    width, kq, k = 48, 16, 10
    dix, six = m.index(dtype=dd), m.sparse_index(width, sd)
    assert dix.add_texts(texts) == 0 and six.add_texts(texts) == 0 and len(dix) == len(six) == len(texts)
    q = m.encode_batch(queries)
    q_ids, q_w = m.encode_sparse(queries, kq)
    for wd, ws in ((1.0, 1.0), (0.3, 0.01)):
        got = dix.hybrid_search_texts(six, queries, kq, k, wd, ws)
        assert _same(got, dix.hybrid_search(six, q, q_ids, q_w, k, wd, ws)), (wd, ws)
        assert (got[0] >= 0).all()
    # one text at a time is the same text in the batch
    one = dix.hybrid_search_texts(six, queries[3:4], kq, k, 0.3, 0.01)
    assert _same(one, (got[0][3:4], got[1][3:4]))
    # a sparse side whose model has no head is refused, outputs untouched; so is a dense side of another dim
    plain = pybert.BertModel(without)
    six2 = plain.sparse_index(width, sd, n_vocab=m.n_vocab)
    out_i, out_s = np.full((1, 4), 7, np.int32), np.full((1, 4), 7.0, np.float32)
    txt = (C.c_char_p * 1)(b"a text")
    few = m.index(dtype=dd)
    capfd.readouterr()
    assert m.lib.bert_hip_hybrid_search_texts(few.ix, six2.ix, 1, 1, txt, 4, 1.0, 1.0, 4, _p(out_i), _p(out_s)) == -2
    assert "no MLM head" in capfd.readouterr().err
    odd = m.index(dim=m.n_embd + 1, dtype=dd)
    empty = m.sparse_index(width, sd)
    assert m.lib.bert_hip_hybrid_search_texts(odd.ix, empty.ix, 1, 1, txt, 4, 1.0, 1.0, 4, _p(out_i), _p(out_s)) == -2
    assert "dim" in capfd.readouterr().err
    assert (out_i == 7).all() and (out_s == 7.0).all()
    with pytest.raises(ValueError):
        few.hybrid_search_texts(six2, ["a text"], 4, 4)
    for x in (dix, six, six2, few, odd, empty):
        x.close()
    plain.close()
    m.close()


# ------------------------------------------------------------------------------------------------
# 8. stream capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dd, sd", [("f16", "f32"), ("i8", "f16")])
def test_a_reserved_device_call_is_captured_and_replayed(model, hip, dd, sd, masked):
    name = N4200
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    nq, k = 9, 10
    dix, six = model.index(c.dim, dd), model.sparse_index(c.width, sd, n_vocab=c.V)
    dix.hybrid_reserve(six, c.n, nq, k)
    dix.add(rows)
    six.add(ids, w)
    qual, words, live = None, None, np.ones(c.n, bool)
    if masked:
        gone_d, gone_s = np.arange(5, c.n, 7, dtype=np.int32), np.arange(3, c.n, 11, dtype=np.int32)
        dix.remove(gone_d)
        six.remove(gone_s)
        live[gone_d] = False
        live[gone_s] = False
        qual = lc._patterns(c.n)["random 50 %"]
        words = pybert.allow_words(qual, c.n)
    d_q, d_qi, d_qw = hip.upload(np.array(queries[:nq])), hip.upload(np.array(q_ids[:nq])), hip.upload(np.array(q_w[:nq]))
    d_allow = hip.upload(words) if masked else 0
    d_i, d_s = hip.nans((nq, k), np.int32), hip.nans((nq, k))
    s = hip.stream()
    call = lambda stream: model.lib.bert_hip_hybrid_search_device(dix.ix, six.ix, nq, d_q, c.kq, d_qi, d_qw, 0.7, 0.3, d_allow or None,
                                                                  len(words) if masked else 0, k, d_i, d_s, stream)
    with hip.capture(s) as cap:
        r = call(s)
    assert r == 0 and cap.status == OK and cap.graph
    assert (hip.download(d_i, (nq, k), np.int32) == -1).all(), "capturing must run nothing"
    # the dense queries' ingest (i8: one kernel as well), scores, query images, hybrid scan, merge — and the bitmap's AND in front
    assert hip.kernel_nodes(cap.graph) == 5 + int(masked)
    ex = hip.instantiate(cap.graph)
    for step, lo in enumerate((0, 12)):
        # new queries written into the same buffers; each replay equals the eager call and the reference
        hip.write(d_q, np.array(queries[lo:lo + nq]))
        hip.write(d_qi, np.array(q_ids[lo:lo + nq]))
        hip.write(d_qw, np.array(q_w[lo:lo + nq]))
        hip.poison(d_i, (nq, k), np.int32)
        hip.poison(d_s, (nq, k))
        hip.launch(ex, s)
        got = hip.download(d_i, (nq, k), np.int32), hip.download(d_s, (nq, k))
        hip.poison(d_i, (nq, k), np.int32)
        assert call(None) == 0
        assert _same(got, (hip.download(d_i, (nq, k), np.int32), hip.download(d_s, (nq, k)))), step
        assert _same(got, _want(model, name, dd, sd, live if qual is None else live & qual, 0.7, 0.3, k, slice(lo, lo + nq))), step
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_q, d_qi, d_qw, d_i, d_s, *([d_allow] if masked else []))
    dix.close()
    six.close()


def test_capturing_an_unreserved_call_fails_cleanly(model, hip, capfd):
    """As test_gpu_stream_capture.py's control: the call has to size the hybrid workspace inside the capture, which the header calls
    illegal: it returns an error after a line on stderr, the capture ends without a graph, nothing ran — and the indexes go on."""
    name = N300
    c = CASES[name]
    rows, queries, ids, w, q_ids, q_w = _data(name)
    dix, six = _pair(model, name, "f16", "f32")
    want = dix.hybrid_search(six, queries[:2], q_ids[:2], q_w[:2], 5)                # (sized for 2 queries: 65 need more)
    d_q, d_qi, d_qw = hip.upload(np.array(queries)), hip.upload(np.array(q_ids)), hip.upload(np.array(q_w))
    d_i, d_s = hip.nans((c.nq, 5), np.int32), hip.nans((c.nq, 5))
    s = hip.stream()
    capfd.readouterr()
    with hip.capture(s) as cap:
        r = model.lib.bert_hip_hybrid_search_device(dix.ix, six.ix, c.nq, d_q, c.kq, d_qi, d_qw, 1.0, 1.0, None, 0, 5, d_i, d_s, s)
    err = capfd.readouterr().err
    seen = f"the call returned {r} ({err.strip()!r}), hipStreamEndCapture {cap.status}, graph {cap.graph}"
    assert r == -3 and "bert_hip_hybrid_search_device" in err, seen
    assert cap.status != OK and not cap.graph, seen
    assert (hip.download(d_i, (c.nq, 5), np.int32) == -1).all()
    hip.destroy_stream(s)
    assert _same(dix.hybrid_search(six, queries[:2], q_ids[:2], q_w[:2], 5), want)
    full = dix.hybrid_search(six, queries, q_ids, q_w, 5)
    assert _same(full, _want(model, name, "f16", "f32", None, 1.0, 1.0, 5))
    hip.free(d_q, d_qi, d_qw, d_i, d_s)
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 9. bert-search --hybrid
# ------------------------------------------------------------------------------------------------
def test_bert_search_hybrid_agrees_with_the_binding(text_model, tmp_path):
    path, without, words = text_model
    rng = np.random.default_rng(8)
    lines = [" ".join(rng.choice(words, size=int(n), replace=False)) for n in rng.integers(3, 12, size=12)]
    assert len(set(lines)) == 12
    file = tmp_path / "lines.txt"
    file.write_text("\n".join(lines) + "\n")
    width, k = 32, 5
    exe = os.path.join(BIN, "bert-search")
    base = [exe, "-m", path, "-f", str(file), "--hybrid", path, "--sparse-width", str(width), "--weights", "0.5,0.25", "-k", str(k)]
    r = subprocess.run(base, input="\n".join(lines) + "\nq\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Loaded 12 lines." in r.stdout
    blocks = r.stdout.split("Closest texts:\n")[1:]
    assert len(blocks) == 12
    m = pybert.BertModel(path)
    dix, six = m.index(), m.sparse_index(width, "f32")
    dix.add_texts(lines)
    six.add_texts(lines)
    ids, sc = dix.hybrid_search_texts(six, lines, width, k, 0.5, 0.25)
    for i, block in enumerate(blocks):
        found = [lines.index(l.split(". ", 1)[1]) for l in block.splitlines() if l[:1].isdigit() and ". " in l]
        shown = [float(l.split(": ")[1].rstrip(")")) for l in block.splitlines() if l.startswith(" (similarity score: ")]
        assert len(found) == k and found == ids[i].tolist(), (i, found, ids[i])
        assert np.allclose(shown, sc[i], rtol=0, atol=6e-5 + 1e-6 * np.abs(sc[i]).max())        # printed with 4 decimals
    dix.close()
    six.close()
    m.close()
    # the combinations the usage text excludes exit with status 2
    for extra in (["--sparse"], ["--lists", "4"], ["--rescore", "20"], ["--long"], ["--maxsim"], ["--cross"]):
        bad = subprocess.run(base + extra, input="q\n", capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and "--hybrid" in bad.stderr, (extra, bad.returncode, bad.stderr)
    bad = subprocess.run(base[:-4] + ["--weights", "1,nan"], input="q\n", capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2, bad.stderr
