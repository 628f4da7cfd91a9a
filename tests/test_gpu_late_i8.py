"""The token index's int8 form on the GPU (include/bert_hip.h "TOKEN INDEX, int8 form").  The oracle is token_i8_reference.scores_i8, the
header's score restated in NumPy float32 — every step of it is exact or one correctly rounded operation in a stated order, so ids must be
equal and scores equal in bits where they are not zero (token_index_reference.same_result): there is no allowance.  The scores are also
held against the float64 MaxSim of the UNQUANTISED rows within the bound token_i8_reference derives, the worst fraction printed.

The rows of a case are f16 values (as f32), so that the host entries (which quantise f32 rows as they are) and the device entries (f16
rows) are given the same values; the stored-form test adds rows that are not."""
import os
import subprocess

import numpy as np
import pytest

import maxsim_reference as mr
import token_i8_reference as t8
import token_index_reference as tref
from bert_cpp_amd import pybert
from hip_graph import Hip

from conftest import ROOT
from test_gpu_long_text import text_model  # noqa: F401  (fixture: the `tiny` dims with a vocabulary of real words)
from test_gpu_token_index import LINES, QUERIES

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
N_DOCS = 300
DIMS = [8, 24, 40, 128, 384, 1024]
QUERY_LENS = [1, 31, 32, 33, 64, 96, 128]
_WORST = {}


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.set_option("token_index_slices", "0")
    m.close()


def _as_f16(rows):
    return np.ascontiguousarray(rows, dtype=np.float32).astype(np.float16).astype(np.float32)


_CASES = {}


def _case(dim):
    """documents, queries (f16 values), the oracle's score matrix and the float64 one of a dim, made once and left unchanged"""
    if dim not in _CASES:
        rng = np.random.default_rng(8000 + dim)
        d32, dcu = tref.documents(rng, N_DOCS, dim)
        q, qcu, _ = mr.packed_set(rng, QUERY_LENS, dim)
        d, q = _as_f16(d32), _as_f16(q)
        S = t8.scores_i8(q, qcu, d, dcu)
        assert S.shape == (len(qcu) - 1, N_DOCS) and np.isfinite(S).all()
        for a in (d32, d, q, S):
            a.setflags(write=False)
        _CASES[dim] = dict(d32=d32, d=d, dcu=dcu, q=q, qcu=qcu, S=S, f64=t8.scores_f64(q, qcu, d, dcu))
    return _CASES[dim]


def _index(model, dim, d, dcu):
    ix = model.token_index(dim, "i8")
    assert ix.add(d, dcu) == 0 and len(ix) == len(dcu) - 1 and ix.n_tokens() == int(dcu[-1] - dcu[0])
    return ix


def _hold_f64(got, f64, what):
    """the returned scores against float64 within the bound; records the worst fraction"""
    ids, sc = got
    want, bound = f64
    worst = 0.0
    for q in range(len(ids)):
        sel = ids[q] >= 0
        err = np.abs(sc[q][sel].astype(np.float64) - want[q, ids[q][sel]])
        b = bound[q, ids[q][sel]]
        assert (err <= b).all(), (what, q)
        worst = max(worst, float((err / b).max()) if sel.any() else 0.0)
    _WORST[what] = max(_WORST.get(what, 0.0), worst)
    print(f"{what}: worst fraction of the float64 bound {worst:.3f}")


def _f16(hip, rows):
    return hip.upload(np.ascontiguousarray(rows, dtype=np.float32).astype(np.float16))


def _device_search(hip, ix, q, qcu, max_q_len, k, words=None, stream=0):
    nq = len(qcu) - 1
    d_q, d_qcu = _f16(hip, q), hip.upload(np.asarray(qcu, np.int32))
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
    d_w = hip.upload(words) if words is not None else None
    try:
        ix.search_device(nq, d_qcu, d_q, max_q_len, k, d_ids, d_sc, stream, d_w, 0 if words is None else len(words))
    finally:
        out = hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32)
        hip.free(d_q, d_qcu, d_ids, d_sc, *([d_w] if d_w else []))
    return out


def _device_rescore(hip, ix, q, qcu, cand, k):
    nq = len(qcu) - 1
    cand = np.ascontiguousarray(cand, dtype=np.int32).reshape(nq, -1)
    d_q, d_qcu, d_c = _f16(hip, q), hip.upload(np.asarray(qcu, np.int32)), hip.upload(cand)
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
    ix.rescore_device(nq, d_qcu, d_q, cand.shape[1], d_c, k, d_ids, d_sc)
    out = hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32)
    hip.free(d_q, d_qcu, d_c, d_ids, d_sc)
    return out


def _expected(S, qual, k):
    """the search over the documents qual (bool [n_docs]) alone"""
    Sm = np.array(S, dtype=np.float32)
    Sm[:, ~np.asarray(qual, dtype=bool)] = np.nan
    return tref.search_expected(Sm, k)


def _same_codes(ix, doc, rows):
    codes, scales = ix.get_codes(doc)
    wc, ws = t8.quantise(rows)
    return np.array_equal(codes, wc) and np.array_equal(scales.view(np.uint32), ws.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# the stored form
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_the_stored_form_is_the_references(model, dim):
    c = _case(dim)
    d32, dcu = c["d32"], c["dcu"]
    hip = Hip()
    docs = (0, 2, 9, 128, N_DOCS - 1)
    doc = lambda rows, i: rows[dcu[i]:dcu[i + 1]]
    # add: the f32 rows as they are (they are not f16 values)
    assert not np.array_equal(d32, _as_f16(d32))
    ix = _index(model, dim, d32, dcu)
    assert ix.dtype == "i8" and model.lib.bert_hip_late_index_dtype(ix.ix) == 2
    for i in docs:
        assert _same_codes(ix, i, doc(d32, i)), i
        codes, scales = ix.get_codes(i)
        assert codes.shape == (dcu[i + 1] - dcu[i], t8.dpad(dim)) and not codes[:, dim:].any()
        want = codes[:, :dim].astype(np.float32) * scales[:, None]
        assert np.array_equal(ix.get_doc(i).view(np.uint32), want.view(np.uint32)), i
    with pytest.raises(ValueError):
        ix.get_codes(N_DOCS)
    # a short capacity writes nothing
    codes, scales = np.full((1, t8.dpad(dim)), 7, np.int8), np.full(1, 7.0, np.float32)
    assert model.lib.bert_hip_late_index_get_codes(ix.ix, 9, codes.ctypes.data, scales.ctypes.data, 1) == dcu[10] - dcu[9] > 1
    assert (codes == 7).all() and (scales == 7.0).all()
    ix.close()
    # add_device: f16 rows; an add in three pieces, the storage growing between them
    dev, pieces = model.token_index(dim, "i8"), model.token_index(dim, "i8")
    d_rows = _f16(hip, d32)
    assert dev.add_device(dcu, d_rows) == 0
    hip.sync()
    a, b = 7, 130
    assert pieces.add(d32[:dcu[a]], dcu[:a + 1]) == 0 and pieces.add_device(dcu[a:b + 1], d_rows) == a
    hip.sync()
    assert pieces.add(d32[dcu[b]:], dcu[b:] - dcu[b]) == b and len(pieces) == N_DOCS and pieces.n_tokens() == int(dcu[-1])
    for i in docs:
        assert _same_codes(dev, i, _as_f16(doc(d32, i))), i
        assert _same_codes(pieces, i, _as_f16(doc(d32, i)) if a <= i < b else doc(d32, i)), i
    hip.free(d_rows)
    dev.close(); pieces.close()


# ------------------------------------------------------------------------------------------------
# search
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_search_against_the_reference(model, dim):
    c = _case(dim)
    hip = Hip()
    ix = _index(model, dim, c["d"], c["dcu"])
    assert ix.max_query_tokens() == 128 and int(np.diff(c["qcu"]).max()) == 128
    for k in (1, 10, 256):
        got = ix.search(c["q"], c["qcu"], k)
        assert tref.same_result(got, tref.search_expected(c["S"], k)), (dim, k)
        _hold_f64(got, c["f64"], f"int8 search dim {dim}")
    # a query of 129 tokens is refused, the outputs untouched
    too_long = _as_f16(mr.unit_rows(np.random.default_rng(1), 129, dim))
    with pytest.raises(ValueError):
        ix.search(too_long, [0, 129], 4)
    ids, sc = np.full((1, 4), 7, np.int32), np.full((1, 4), 7.0, np.float32)
    cu = np.array([0, 129], np.int32)
    assert model.lib.bert_hip_token_index_search(ix.ix, 1, cu.ctypes.data, too_long.ctypes.data, 4, ids.ctypes.data, sc.ctypes.data) == -2
    assert (ids == 7).all() and (sc == 7.0).all()
    d_ids, d_sc, d_q, d_cu = hip.nans((1, 4), np.int32), hip.nans((1, 4), np.float32), _f16(hip, too_long), hip.upload(cu)
    before = hip.download(d_ids, (1, 4), np.int32), hip.download(d_sc, (1, 4), np.float32)
    with pytest.raises(ValueError):
        ix.search_device(1, d_cu, d_q, 129, 4, d_ids, d_sc)
    after = hip.download(d_ids, (1, 4), np.int32), hip.download(d_sc, (1, 4), np.float32)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(before, after))
    hip.free(d_ids, d_sc, d_q, d_cu)
    ix.close()


def test_small_and_empty_indexes(model):
    c = _case(24)
    hip = Hip()
    for n in (1, 3):
        ix = _index(model, 24, c["d"], c["dcu"][:n + 1])
        got = ix.search(c["q"], c["qcu"], 10)
        assert tref.same_result(got, tref.search_expected(c["S"][:, :n], 10))
        ix.close()
    ix = model.token_index(24, "i8")
    for got in (ix.search(c["q"], c["qcu"], 5), _device_search(hip, ix, c["q"], c["qcu"], 128, 5),
                ix.rescore(c["q"], c["qcu"], np.full((len(c["qcu"]) - 1, 3), -1), 5)):
        assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    assert ix.search(np.zeros((0, 24), np.float32), [0], 5)[0].shape == (0, 5)
    ix.close()


# ------------------------------------------------------------------------------------------------
# independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [40, 384])
def test_a_result_depends_on_the_query_and_the_documents_alone(model, dim):
    c = _case(dim)
    q, qcu, d, dcu = c["q"], c["qcu"], c["d"], c["dcu"]
    nq = len(qcu) - 1
    hip = Hip()
    ix = _index(model, dim, d, dcu)
    base = ix.search(q, qcu, 256)
    assert tref.same_result(base, tref.search_expected(c["S"], 256))
    same = lambda got, k=256: tref.same_result(got, (base[0][:, :k], base[1][:, :k]))
    every = np.tile(np.arange(N_DOCS, dtype=np.int32), (nq, 1))
    # how the scan (and the rescore's walk of its lists) is cut
    for slices in (1, 7, 4096):
        model.set_option("token_index_slices", str(slices))
        assert same(ix.search(q, qcu, 256)), slices
        assert same(ix.rescore(q, qcu, every, 256)), slices
    model.set_option("token_index_slices", "0")
    # top-10 and top-100 are prefixes; a query alone is the query in the batch
    assert same(ix.search(q, qcu, 10), 10) and same(ix.search(q, qcu, 100), 100)
    for i in range(nq):
        alone = ix.search(q[qcu[i]:qcu[i + 1]], [0, qcu[i + 1] - qcu[i]], 10)
        assert tref.same_result(alone, (base[0][i:i + 1, :10], base[1][i:i + 1, :10])), i
    # host against device entry; search against rescore of all ids, host and device
    assert same(_device_search(hip, ix, q, qcu, 128, 256))
    assert same(ix.rescore(q, qcu, every, 256)) and same(_device_rescore(hip, ix, q, qcu, every, 256))
    ix.close()
    # after growth: one add per document from an index of the first capacity; reserved storage filled from the device
    grown = model.token_index(dim, "i8")
    for i in range(N_DOCS):
        assert grown.add(d[dcu[i]:dcu[i + 1]], [0, dcu[i + 1] - dcu[i]]) == i
    assert same(grown.search(q, qcu, 256))
    grown.close()
    dev = model.token_index(dim, "i8")
    dev.reserve(N_DOCS, int(dcu[-1]), nq, 128, 256)
    d_rows = _f16(hip, d)
    half = N_DOCS // 2
    assert dev.add_device(dcu[:half + 1], d_rows) == 0 and dev.add_device(dcu[half:], d_rows) == half
    hip.sync()
    assert same(dev.search(q, qcu, 256))
    hip.free(d_rows)
    dev.close()


# ------------------------------------------------------------------------------------------------
# ties
# ------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_ids_across_slices_steps_and_waves(model):
    """the same document stored at ids far apart: with 7 slices of 86 the copies lie in slices 0, 1, 3, 5, 6, in the first and the second
    step of a slice, and meet different waves ((id - slice start) % 4 = 3, 0, 1, 3, 2); k cuts through the tie"""
    dim, n = 8, 600
    rng = np.random.default_rng(77)
    q, qcu, _ = mr.packed_set(rng, [33], dim)
    q = _as_f16(q)
    lens = [tref.DOC_LENS[i % 5] for i in range(n)]
    copies = [3, 86, 259, 433, 598]
    parts = [_as_f16(mr.unit_rows(rng, ln, dim)) for ln in lens]
    for i in copies:
        parts[i] = q.copy()
        lens[i] = len(q)
    d, dcu = np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    S = t8.scores_i8(q, qcu, d, dcu)
    assert len(set(S[0, copies].tolist())) == 1 and (np.delete(S[0], copies) < S[0, 3]).all()
    ix = _index(model, dim, d, dcu)
    for slices in ("0", "7", "1", "600"):
        model.set_option("token_index_slices", slices)
        for k, want in ((1, [3]), (3, [3, 86, 259]), (5, copies)):
            got = ix.search(q, qcu, k)
            assert got[0][0].tolist() == want, (slices, k)
            assert tref.same_result(got, tref.search_expected(S, k))
    model.set_option("token_index_slices", "0")
    ix.close()


# ------------------------------------------------------------------------------------------------
# masking
# ------------------------------------------------------------------------------------------------
def test_removals_and_allow_lists_against_the_reference_on_the_subset(model):
    c = _case(40)
    q, qcu, S, n = c["q"], c["qcu"], c["S"], N_DOCS
    nq = len(qcu) - 1
    hip = Hip()
    rng = np.random.default_rng(31)
    doc = np.arange(n)
    patterns = {"a step of 64 cleared between two full ones": ~((doc >= 64) & (doc < 128)),
                "one document per step": doc % 64 == 5, "only wave 2": doc % 4 == 2, "random 50 %": rng.random(n) < 0.5,
                "none": np.zeros(n, bool), "fewer than k": np.isin(doc, [1, 77, 299])}
    plain = _index(model, 40, c["d"], c["dcu"])
    for name, qual in patterns.items():
        r = rng.random(n) < 0.5
        removed, both = _index(model, 40, c["d"], c["dcu"]), _index(model, 40, c["d"], c["dcu"])
        assert removed.remove(np.flatnonzero(~qual)) == int((~qual).sum()) and removed.n_live() == int(qual.sum())
        assert removed.n_live_tokens() == int(np.diff(c["dcu"])[qual].sum()) and len(removed) == n
        both.remove(np.flatnonzero(~(qual | r)))
        # (7 slices of 43 documents: slices start inside a mask word; 4096: one document per slice)
        for slices in ("0", "1", "7", "4096"):
            model.set_option("token_index_slices", slices)
            for k in (1, 10, 256):
                want = _expected(S, qual, k)
                for mode, ix, allow in (("allow", plain, qual), ("removed", removed, None), ("both", both, qual | ~r)):
                    assert tref.same_result(ix.search(q, qcu, k, allow=allow), want), (name, mode, slices, k)
        model.set_option("token_index_slices", "7")
        words = pybert.allow_words(qual, n)
        assert tref.same_result(_device_search(hip, plain, q, qcu, 128, 10, words), _expected(S, qual, 10)), name
        assert tref.same_result(_device_search(hip, removed, q, qcu, 128, 10), _expected(S, qual, 10)), name
        model.set_option("token_index_slices", "0")
        # rescore skips a removed id, and an id out of range on the device
        cand = rng.integers(-1, n, (nq, 70)).astype(np.int32)
        Sm = np.array(S)
        Sm[:, ~qual] = np.nan
        assert tref.same_result(removed.rescore(q, qcu, cand, 10), tref.rescore_expected(Sm, cand, 10)), name
        wild = cand.copy()
        wild[:, 3], wild[:, 7], wild[:, 11] = n, -7, 2 ** 31 - 1
        assert tref.same_result(_device_rescore(hip, removed, q, qcu, wild, 10), tref.rescore_expected(Sm, wild, 10)), name
        with pytest.raises(ValueError):
            removed.rescore(q, qcu, wild, 10)
        removed.close(); both.close()
    assert tref.same_result(plain.search(q, qcu, 10), tref.search_expected(S, 10))
    # a repeated id counts each time it appears
    got = plain.rescore(q[:qcu[1]], qcu[:2], [[7, 7, 2, 7]], 6)
    assert sorted(got[0][0].tolist()) == [-1, -1, 2, 7, 7, 7] and tref.same_result(got, tref.rescore_expected(S[:1], [[7, 7, 2, 7]], 6))
    plain.close()


# ------------------------------------------------------------------------------------------------
# non-finite and large rows
# ------------------------------------------------------------------------------------------------
def test_non_finite_rows_are_never_returned_and_leave_their_neighbours(model):
    c = _case(24)
    q, qcu, dcu = c["q"], c["qcu"], c["dcu"]
    nq = len(qcu) - 1
    d = np.array(c["d"])
    inf_doc, nan_doc = 7, 128                                           # 96 and 130 tokens: the bad token in a later block of 32
    d[dcu[inf_doc] + 40, 3] = np.inf
    d[dcu[nan_doc + 1] - 1, 0] = np.nan
    S = t8.scores_i8(q, qcu, d, dcu)
    ok = np.ones(N_DOCS, bool)
    ok[[inf_doc, nan_doc]] = False
    assert np.isnan(S[:, ~ok]).all() and np.array_equal(S[:, ok].view(np.uint32), c["S"][:, ok].view(np.uint32))
    ix = _index(model, 24, d, dcu)
    codes, scales = ix.get_codes(inf_doc)
    assert np.isnan(scales[40]) and not codes[40].any() and np.isfinite(np.delete(scales, 40)).all()
    for k in (10, 256):
        got = ix.search(q, qcu, k)
        assert not np.isin(got[0], [inf_doc, nan_doc]).any()
        assert tref.same_result(got, _expected(c["S"], ok, k)), k
    every = np.tile(np.arange(N_DOCS, dtype=np.int32), (nq, 1))
    assert tref.same_result(ix.rescore(q, qcu, every, 256), _expected(c["S"], ok, 256))
    # a query with a NaN token gets -1 / -inf; its batch neighbours keep their bits
    qb = np.concatenate([q[qcu[3]:qcu[4]], q[qcu[4]:qcu[5]], q[qcu[1]:qcu[2]]])
    qbcu = np.array([0, 33, 97, 128], np.int32)
    qb[33 + 50, 2] = np.nan
    for got in (ix.search(qb, qbcu, 10), ix.rescore(qb, qbcu, every[:3], 10)):
        assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()
        assert tref.same_result((got[0][[0, 2]], got[1][[0, 2]]), _expected(c["S"][[3, 1]], ok, 10))
    ix.close()


def test_large_rows_do_not_leak_into_their_neighbours(model):
    """rows of magnitude 6e4 (the largest f16 values) beside unit rows: every token has its own scale"""
    dim = 24
    rng = np.random.default_rng(9)
    q, qcu, _ = mr.packed_set(rng, [33, 31], dim)
    q = _as_f16(q)
    targets = [_as_f16(mr.unit_rows(rng, n, dim)) for n in (1, 31, 33, 65)]
    loud = lambda n: _as_f16(6e4 * q[rng.integers(0, len(q), n)] / np.abs(q).max())
    docs = []
    for t in targets:
        docs += [loud(33), t]
    docs.append(loud(5))
    cu_of = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32)
    quiet_d, quiet_cu, loud_d, loud_cu = np.concatenate(targets), cu_of(targets), np.concatenate(docs), cu_of(docs)
    assert np.isfinite(loud_d).all() and np.abs(loud_d).max() > 5e4
    Sq, Sl = t8.scores_i8(q, qcu, quiet_d, quiet_cu), t8.scores_i8(q, qcu, loud_d, loud_cu)
    assert np.array_equal(Sl[:, 1::2].view(np.uint32), Sq.view(np.uint32)) and np.isfinite(Sl).all()
    a, b = _index(model, dim, quiet_d, quiet_cu), _index(model, dim, loud_d, loud_cu)
    quiet, noisy = a.search(q, qcu, 4), b.search(q, qcu, 9)
    assert tref.same_result(quiet, tref.search_expected(Sq, 4)) and tref.same_result(noisy, tref.search_expected(Sl, 9))
    # a query between loud queries
    lq = [loud(32), q[qcu[0]:qcu[1]], loud(64), q[qcu[1]:qcu[2]], loud(1)]
    among = a.search(np.concatenate(lq), cu_of(lq), 4)
    assert tref.same_result((among[0][[1, 3]], among[1][[1, 3]]), quiet)
    a.close(); b.close()
    # all-negative similarities: a padded document slot that entered the max as 0 would lift every score to 0
    qn, qncu, dn, dncu = mr.negative_sets(rng, [1, 33, 31, 64], [1, 31, 33, 129, 2, 64, 65], dim)
    qn, dn = _as_f16(qn), _as_f16(dn)
    S = t8.scores_i8(qn, qncu, dn, dncu)
    assert (S < 0).all()
    ix = _index(model, dim, dn, dncu)
    got = ix.search(qn, qncu, 7)
    assert tref.same_result(got, tref.search_expected(S, 7)) and (got[1] < 0).all()
    _hold_f64(got, t8.scores_f64(qn, qncu, dn, dncu), "int8 search negative dim 24")
    ix.close()


# ------------------------------------------------------------------------------------------------
# the device form's guards
# ------------------------------------------------------------------------------------------------
def test_device_guards_give_empty_slots_and_leave_the_neighbours(model):
    c = _case(40)
    hip = Hip()
    ix = _index(model, 40, c["d"], c["dcu"])
    rows = c["q"][:60]
    # queries: 5 tokens | empty | 40 tokens, longer than max_q_len 32 | descending (45 -> 40) | 20 tokens
    qcu = np.array([0, 5, 5, 45, 40, 60], np.int32)
    got = _device_search(hip, ix, rows, qcu, 32, 6)                      # (the outputs are pre-filled with NaN patterns)
    for bad in (1, 2, 3):
        assert (got[0][bad] == -1).all() and np.isneginf(got[1][bad]).all(), bad
    want = ix.search(np.concatenate([rows[:5], rows[40:60]]), [0, 5, 25], 6)
    assert tref.same_result((got[0][[0, 4]], got[1][[0, 4]]), want)
    every = np.tile(np.arange(N_DOCS, dtype=np.int32), (5, 1))
    resc = _device_rescore(hip, ix, rows, qcu, every, 6)
    for bad in (1, 3):
        assert (resc[0][bad] == -1).all() and np.isneginf(resc[1][bad]).all(), bad
    assert tref.same_result((resc[0][[0, 4]], resc[1][[0, 4]]), want)
    # a start below 0
    got = _device_search(hip, ix, rows, np.array([-3, 5, 10], np.int32), 32, 6)
    assert (got[0][0] == -1).all() and np.isneginf(got[1][0]).all()
    assert tref.same_result((got[0][1:], got[1][1:]), ix.search(rows[5:10], [0, 5], 6))
    # a rescore's query of more than 128 tokens: the host form refuses it, the device form gives it empty slots
    long_q = _as_f16(mr.unit_rows(np.random.default_rng(2), 129 + 5, 40))
    with pytest.raises(ValueError):
        ix.rescore(long_q, [0, 129, 134], every[:2], 6)
    resc = _device_rescore(hip, ix, long_q, [0, 129, 134], every[:2], 6)
    assert (resc[0][0] == -1).all() and np.isneginf(resc[1][0]).all()
    assert tref.same_result((resc[0][1:], resc[1][1:]), ix.search(long_q[129:], [0, 5], 6))
    ix.close()


# ------------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------------
def test_search_and_rescore_are_captured_and_replayed(model):
    c = _case(128)
    q, qcu, S = c["q"], c["qcu"], c["S"]
    nq, k, n_cand = len(qcu) - 1, 10, 33
    hip = Hip()
    ix = model.token_index(128, "i8")
    ix.reserve(N_DOCS, int(c["dcu"][-1]), nq, 128, k)
    assert ix.add(c["d"], c["dcu"]) == 0
    cand = np.random.default_rng(8).integers(-1, N_DOCS, (nq, n_cand)).astype(np.int32)
    d_q, d_qcu, d_c = _f16(hip, q), hip.upload(qcu), hip.upload(cand)
    outs = [hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32), hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)]
    s = hip.stream()
    # eager first: the results to compare with, and the rescore workspace of this shape
    ix.search_device(nq, d_qcu, d_q, 128, k, outs[0], outs[1], s)
    ix.rescore_device(nq, d_qcu, d_q, n_cand, d_c, k, outs[2], outs[3], s)
    read = lambda: [hip.download(p, (nq, k), np.int32 if i % 2 == 0 else np.float32) for i, p in enumerate(outs)]
    eager = read()
    assert tref.same_result(eager[:2], tref.search_expected(S, k)) and tref.same_result(eager[2:], tref.rescore_expected(S, cand, k))
    with hip.capture(s) as cap:
        ix.search_device(nq, d_qcu, d_q, 128, k, outs[0], outs[1], s)
        ix.rescore_device(nq, d_qcu, d_q, n_cand, d_c, k, outs[2], outs[3], s)
    assert cap.status == 0 and cap.graph and hip.kernel_nodes(cap.graph) == 6          # twice: quantise, scan, merge
    ex = hip.instantiate(cap.graph)
    for _ in range(2):
        for i, p in enumerate(outs):
            hip.poison(p, (nq, k), np.int32 if i % 2 == 0 else np.float32)
        hip.launch(ex, s)
        replay = read()
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(replay, eager))
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_q, d_qcu, d_c, *outs)
    ix.close()


# ------------------------------------------------------------------------------------------------
# the f16 form, the refused operations
# ------------------------------------------------------------------------------------------------
def test_the_f16_form_through_the_new_create_is_the_f16_form(model):
    c = _case(40)
    old = model.token_index(40)
    new = pybert.BertTokenIndex.__new__(pybert.BertTokenIndex)            # an index of bert_hip_late_index_create(ctx, 40, 1)
    new.model, new.lib, new.dim, new.dtype = model, model.lib, 40, "f16"
    new.ix = model.lib.bert_hip_late_index_create(model.ctx, 40, 1)
    assert new.ix and model.lib.bert_hip_late_index_dtype(new.ix) == 1 and model.lib.bert_hip_late_index_dtype(old.ix) == 1
    assert old.dtype == "f16" and old.max_query_tokens() == new.max_query_tokens() == tref.max_query_tokens(40)
    for ix in (old, new):
        assert ix.add(c["d32"], c["dcu"]) == 0
    a, b = old.search(c["q"], c["qcu"], 256), new.search(c["q"], c["qcu"], 256)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert tref.same_result(a, tref.search_expected(model.maxsim(c["q"], c["qcu"], c["d32"], c["dcu"]), 256))
    assert np.array_equal(old.get_doc(9).view(np.uint32), new.get_doc(9).view(np.uint32))
    for ix in (old, new):
        with pytest.raises(ValueError):
            ix.get_codes(0)
    assert not model.lib.bert_hip_late_index_create(model.ctx, 40, 0) and not model.lib.bert_hip_late_index_create(model.ctx, 40, 3)
    old.close(); new.close()


def test_compact_and_save_are_refused_and_the_index_goes_on(model, tmp_path):
    c = _case(40)
    ix = _index(model, 40, c["d"], c["dcu"])
    ix.remove([3, 250])
    ok = np.ones(N_DOCS, bool)
    ok[[3, 250]] = False
    before = ix.search(c["q"], c["qcu"], 10)
    assert tref.same_result(before, _expected(c["S"], ok, 10))
    with pytest.raises(ValueError):
        ix.compact()
    with pytest.raises(ValueError):
        ix.save(str(tmp_path / "i8.tok"))
    assert not (tmp_path / "i8.tok").exists() and not (tmp_path / "i8.tok.tmp").exists()
    assert len(ix) == N_DOCS and ix.n_live() == N_DOCS - 2
    assert tref.same_result(ix.search(c["q"], c["qcu"], 10), before)
    ix.close()


# ------------------------------------------------------------------------------------------------
# texts and the example
# ------------------------------------------------------------------------------------------------
def test_texts_are_the_f16_token_rows_quantised(text_model):
    m = pybert.BertModel(text_model[0])
    hip = Hip()
    m.set_option("chunk_tokens", "70")           # the lines are cut into several chunks
    ix = m.token_index(dtype="i8")
    assert ix.add_texts(LINES[:5]) == 0 and ix.add_texts(LINES[5:]) == 5 and len(ix) == len(LINES)
    m.set_option("chunk_tokens", "262144")
    rows, cu = m.encode_tokens(LINES, normalize=True)
    assert ix.n_tokens() == int(cu[-1])
    dev = m.token_index(dtype="i8")
    d_rows = _f16(hip, rows)
    assert dev.add_device(cu, d_rows) == 0
    hip.sync()
    for i in range(len(LINES)):
        assert _same_codes(ix, i, _as_f16(rows[cu[i]:cu[i + 1]])), i
        assert all(np.array_equal(x, y) for x, y in zip(ix.get_codes(i), dev.get_codes(i))), i
    qrows, qcu = m.encode_tokens(QUERIES, normalize=True)
    want = _device_search(hip, dev, qrows, qcu, 128, 5)
    got = ix.search_texts(QUERIES, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert tref.same_result(got, tref.search_expected(t8.scores_i8(_as_f16(qrows), qcu, _as_f16(rows), cu), 5))
    hip.free(d_rows)
    dev.close(); ix.close(); m.close()


def test_bert_search_late_i8_finds_a_line_as_its_own_best_match(text_model, tmp_path):
    path, _ = text_model
    lines = [l for l in LINES if l]
    f = tmp_path / "lines.txt"
    f.write_text("\n".join(lines) + "\n")
    exe = os.path.join(BIN, "bert-search")
    asked = [lines[3], lines[7]]
    stdin = "".join(q + "\n" for q in asked) + "q\n"
    run = lambda flags: subprocess.run([exe, "-m", path, "-f", str(f), "-k", "3"] + flags, input=stdin, capture_output=True, text=True, timeout=300)
    late = run(["--late", "--i8"])
    assert late.returncode == 0, late.stderr
    m = pybert.BertModel(path)
    ix = m.token_index(dtype="i8")
    ix.add_texts(lines)
    ids, sc = ix.search_texts(asked, 3)
    assert ids[:, 0].tolist() == [3, 7]
    prompt = "Enter a text to find similar texts (enter 'q' to quit): "
    want = f"Loading texts from {f}...\nLoaded {len(lines)} lines.\n"
    for i in range(len(asked)):
        want += prompt + "\nClosest texts:\n" + "".join(f"{j + 1}. {lines[ids[i][j]]}\n (MaxSim score: {sc[i][j]:.4f})\n" for j in range(3))
    assert late.stdout == want + prompt + "\n"
    ix.close(); m.close()
    kept = run(["--maxsim", "8", "--token-index", "--i8"])
    assert kept.returncode == 0 and kept.stdout.count("MaxSim score") == 3 * len(asked), kept.stderr


def test_worst_fractions_are_recorded():
    """(last in the file) every float64 bound above was met: the figures, for the log"""
    for what, frac in sorted(_WORST.items()):
        print(f"{what}: {frac:.3f}")
    assert _WORST and all(f <= 1.0 for f in _WORST.values())
