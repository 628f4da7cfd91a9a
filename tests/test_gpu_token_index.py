"""The token index on the GPU (include/bert_hip.h "TOKEN INDEX").  The oracle for ids and scores is the existing, separately verified
kernel: BertModel.maxsim on all pairs of the same f32 rows, pushed through the reference's order rule (token_index_reference.py).  Ids
must be equal and scores == with equal bits where they are not zero; no id may differ, so there is no allowance.  The scores are also
held against float64 within maxsim_reference's bound, the worst fraction printed."""
import os
import subprocess

import numpy as np
import pytest

import maxsim_reference as mr
import token_index_reference as tref
from bert_cpp_amd import pybert
from hip_graph import Hip

from conftest import ROOT
from test_gpu_long_text import text_model  # noqa: F401  (fixture: the `tiny` dims with a vocabulary of real words)

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
N_DOCS = 300
DIMS = [8, 24, 64, 384, 768, 1024]
_WORST = {}


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.close()


_CASES = {}


def _case(model, dim):
    """documents, queries, the oracle's score matrix and the float64 one of a dim, made once and left unchanged"""
    if dim not in _CASES:
        rng = np.random.default_rng(4000 + dim)
        d, dcu = tref.documents(rng, N_DOCS, dim)
        q, qcu = tref.queries(rng, dim)
        S = model.maxsim(q, qcu, d, dcu)
        assert S.shape == (len(qcu) - 1, N_DOCS) and np.isfinite(S).all()
        _CASES[dim] = dict(d=d, dcu=dcu, q=q, qcu=qcu, S=S, f64=tref.scores_f64(q, qcu, d, dcu))
    return _CASES[dim]


def _index(model, dim, d, dcu):
    ix = model.token_index(dim)
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


def _device_search(hip, ix, q, qcu, max_q_len, k, stream=0):
    nq = len(qcu) - 1
    d_q, d_qcu = _f16(hip, q), hip.upload(np.asarray(qcu, np.int32))
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k), np.float32)
    ix.search_device(nq, d_qcu, d_q, max_q_len, k, d_ids, d_sc, stream)
    out = hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k), np.float32)
    hip.free(d_q, d_qcu, d_ids, d_sc)
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


# ------------------------------------------------------------------------------------------------
# shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_search_against_the_oracle(model, dim):
    c = _case(model, dim)
    ix = _index(model, dim, c["d"], c["dcu"])
    assert ix.max_query_tokens() == tref.max_query_tokens(dim) and int(np.diff(c["qcu"]).max()) == min(128, ix.max_query_tokens())
    for k in (1, 10, 256):
        got = ix.search(c["q"], c["qcu"], k)
        assert tref.same_result(got, tref.search_expected(c["S"], k)), (dim, k)
        _hold_f64(got, c["f64"], f"search dim {dim}")
    # a query one block longer than the scan stages is refused, the outputs untouched
    too_long = mr.unit_rows(np.random.default_rng(1), ix.max_query_tokens() + 1, dim)
    with pytest.raises(ValueError):
        ix.search(too_long, [0, len(too_long)], 4)
    # get_doc: the stored values are the f16 roundings of what was added
    for doc in (0, 9, N_DOCS - 1):
        want = c["d"][c["dcu"][doc]:c["dcu"][doc + 1]].astype(np.float16).astype(np.float32)
        assert np.array_equal(ix.get_doc(doc).view(np.uint32), want.view(np.uint32))
    ix.close()


def test_small_and_empty_indexes(model):
    c = _case(model, 64)
    hip = Hip()
    for n in (1, 3):
        ix = _index(model, 64, c["d"], c["dcu"][:n + 1])
        got = ix.search(c["q"], c["qcu"], 10)
        assert tref.same_result(got, tref.search_expected(c["S"][:, :n], 10))
        assert (got[0][:, n:] == -1).all() and np.isneginf(got[1][:, n:]).all() and (got[0][:, :n] >= 0).all()
        ix.close()
    ix = model.token_index(64)
    assert len(ix) == 0 and ix.n_tokens() == 0
    for got in (ix.search(c["q"], c["qcu"], 5), _device_search(hip, ix, c["q"], c["qcu"], 128, 5),
                ix.rescore(c["q"], c["qcu"], np.full((len(c["qcu"]) - 1, 3), -1), 5)):
        assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    # n_queries == 0: a successful no-op, on an empty and on a filled index
    ids, sc = ix.search(np.zeros((0, 64), np.float32), [0], 5)
    assert ids.shape == (0, 5) and sc.shape == (0, 5)
    assert ix.add(c["d"], c["dcu"][:4]) == 0 and ix.add(c["d"], c["dcu"][:1]) == 3 and len(ix) == 3
    assert ix.search(np.zeros((0, 64), np.float32), [0], 5)[0].shape == (0, 5)
    # refused adds leave the index as it was
    for bad in ([0, 0, 3], [0, 5, 3], [-1, 2]):
        with pytest.raises(ValueError):
            ix.add(c["d"], bad)
    assert len(ix) == 3 and ix.n_tokens() == int(c["dcu"][3])
    with pytest.raises(ValueError):
        ix.search(c["q"], c["qcu"], 257)
    ix.close()


# ------------------------------------------------------------------------------------------------
# ties
# ------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_ids_across_slices_and_waves(model):
    """the same document stored at ids far apart: with 7 slices of 86 the copies lie in slices 0, 1, 3, 5, 6 and meet different waves
    (id - slice start) % 4 = 3, 0, 1, 3, 2); k cuts through the tie"""
    dim, n = 8, 600
    rng = np.random.default_rng(77)
    q, qcu = tref.queries(rng, dim, [33])
    lens = [tref.DOC_LENS[i % 5] for i in range(n)]
    copies = [3, 86, 259, 433, 598]
    parts = [mr.unit_rows(rng, ln, dim) for ln in lens]
    for i in copies:
        parts[i] = q.copy()                      # the query's own tokens: 33 maxima of 1, which no other document reaches
        lens[i] = len(q)
    d, dcu = np.concatenate(parts), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    S = model.maxsim(q, qcu, d, dcu)
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
# independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [24, 384])
def test_a_result_depends_on_the_query_and_the_documents_alone(model, dim):
    c = _case(model, dim)
    q, qcu, d, dcu = c["q"], c["qcu"], c["d"], c["dcu"]
    nq = len(qcu) - 1
    hip = Hip()
    ix = _index(model, dim, d, dcu)
    base = ix.search(q, qcu, 256)
    assert tref.same_result(base, tref.search_expected(c["S"], 256))
    same = lambda got, k=256: tref.same_result(got, (base[0][:, :k], base[1][:, :k]))
    # how the scan is cut
    for slices in (1, 2, 7, N_DOCS):
        model.set_option("token_index_slices", str(slices))
        assert same(ix.search(q, qcu, 256)), slices
    model.set_option("token_index_slices", "0")
    # top-10 is the first 10 of top-256; a query alone is the query among the others
    assert same(ix.search(q, qcu, 10), 10)
    for i in range(nq):
        alone = ix.search(q[qcu[i]:qcu[i + 1]], [0, qcu[i + 1] - qcu[i]], 10)
        assert tref.same_result(alone, (base[0][i:i + 1, :10], base[1][i:i + 1, :10])), i
    # host against device entry point; search against rescore over all ids
    assert same(_device_search(hip, ix, q, qcu, ix.max_query_tokens(), 256))
    every = np.tile(np.arange(N_DOCS, dtype=np.int32), (nq, 1))
    assert same(ix.rescore(q, qcu, every, 256)) and same(_device_rescore(hip, ix, q, qcu, every, 256))
    ix.close()
    # one add per document; add_device; reserved against grown storage
    per_doc = model.token_index(dim)
    for i in range(N_DOCS):
        assert per_doc.add(d[dcu[i]:dcu[i + 1]], [0, dcu[i + 1] - dcu[i]]) == i
    assert same(per_doc.search(q, qcu, 256))
    per_doc.close()
    dev = model.token_index(dim)
    dev.reserve(N_DOCS, int(dcu[-1]), nq, dev.max_query_tokens(), 256)
    d_rows = _f16(hip, d)
    half = N_DOCS // 2
    assert dev.add_device(dcu[:half + 1], d_rows) == 0 and dev.add_device(dcu[half:], d_rows) == half
    hip.sync()
    assert len(dev) == N_DOCS and dev.n_tokens() == int(dcu[-1])
    assert same(dev.search(q, qcu, 256))
    hip.free(d_rows)
    dev.close()


# ------------------------------------------------------------------------------------------------
# neighbours
# ------------------------------------------------------------------------------------------------
def test_loud_neighbours_do_not_leak(model):
    """documents and queries whose rows are 100 x a query token would win any max they leaked into"""
    dim = 24
    rng = np.random.default_rng(9)
    q, qcu = tref.queries(rng, dim, [33, 31])
    targets = [mr.unit_rows(rng, n, dim) for n in (1, 31, 33, 65)]
    loud = lambda n: (100.0 * q[rng.integers(0, len(q), n)]).astype(np.float32)
    quiet_d, quiet_cu = np.concatenate(targets), np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.int32)
    docs = []
    for t in targets:
        docs += [loud(33), t]
    docs.append(loud(5))
    loud_d, loud_cu = np.concatenate(docs), np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int32)
    a, b = _index(model, dim, quiet_d, quiet_cu), _index(model, dim, loud_d, loud_cu)
    quiet = a.search(q, qcu, 4)
    noisy = b.search(q, qcu, 9)
    for i in range(2):
        s_quiet = dict(zip(quiet[0][i].tolist(), quiet[1][i].view(np.uint32).tolist()))
        s_noisy = dict(zip(noisy[0][i].tolist(), noisy[1][i].view(np.uint32).tolist()))
        assert all(s_noisy[2 * t + 1] == s_quiet[t] for t in range(4)), i
        assert set(noisy[0][i, :5].tolist()) == {0, 2, 4, 6, 8}        # the loud documents lead
    # a query between loud queries
    lq = [loud(32), q[qcu[0]:qcu[1]], loud(64), q[qcu[1]:qcu[2]], loud(1)]
    lq_rows, lq_cu = np.concatenate(lq), np.concatenate([[0], np.cumsum([len(x) for x in lq])]).astype(np.int32)
    among = a.search(lq_rows, lq_cu, 4)
    assert tref.same_result((among[0][[1, 3]], among[1][[1, 3]]), quiet)
    a.close(); b.close()
    # all-negative similarities, ordered correctly: a padded document slot that entered the max as 0 would lift every score to 0
    qn, qncu, dn, dncu = mr.negative_sets(rng, [1, 33, 31, 64], [1, 31, 33, 129, 2, 64, 65], dim)
    S = model.maxsim(qn, qncu, dn, dncu)
    assert (S < 0).all()
    ix = _index(model, dim, dn, dncu)
    got = ix.search(qn, qncu, 7)
    assert tref.same_result(got, tref.search_expected(S, 7)) and (got[1] < 0).all()
    _hold_f64(got, tref.scores_f64(qn, qncu, dn, dncu), "search negative dim 24")
    ix.close()


# ------------------------------------------------------------------------------------------------
# the device form's guards
# ------------------------------------------------------------------------------------------------
def test_device_guards_give_empty_slots_and_leave_the_neighbours(model):
    c = _case(model, 64)
    hip = Hip()
    ix = _index(model, 64, c["d"], c["dcu"])
    rows = c["q"][:60]
    # queries: 5 tokens | empty | 40 tokens, longer than max_q_len 32 | descending (45 -> 40) | 20 tokens
    qcu = np.array([0, 5, 5, 45, 40, 60], np.int32)
    got = _device_search(hip, ix, rows, qcu, 32, 6)
    for bad in (1, 2, 3):
        assert (got[0][bad] == -1).all() and np.isneginf(got[1][bad]).all(), bad
    want = ix.search(np.concatenate([rows[:5], rows[40:60]]), [0, 5, 25], 6)
    assert tref.same_result((got[0][[0, 4]], got[1][[0, 4]]), want)
    # a start below 0
    got = _device_search(hip, ix, rows, np.array([-3, 5, 10], np.int32), 32, 6)
    assert (got[0][0] == -1).all() and np.isneginf(got[1][0]).all()
    assert tref.same_result((got[0][1:], got[1][1:]), ix.search(rows[5:10], [0, 5], 6))
    # max_q_len beyond what the scan stages is refused, the outputs untouched
    with pytest.raises(ValueError):
        _device_search(hip, ix, rows, qcu, ix.max_query_tokens() + 1, 6)
    ix.close()


# ------------------------------------------------------------------------------------------------
# rescore
# ------------------------------------------------------------------------------------------------
def test_rescore_candidates(model):
    c = _case(model, 64)
    q, qcu, S = c["q"], c["qcu"], c["S"]
    nq = len(qcu) - 1
    hip = Hip()
    ix = _index(model, 64, c["d"], c["dcu"])
    rng = np.random.default_rng(5)
    for n_cand in (1, 33, 1024):
        cand = rng.integers(-1, N_DOCS, (nq, n_cand)).astype(np.int32)           # -1 entries and, from 33 on, repeated ids
        cand[0, 0] = -1
        for k in (1, 10, 256):
            want = tref.rescore_expected(S, cand, k)
            assert tref.same_result(ix.rescore(q, qcu, cand, k), want), (n_cand, k)
            assert tref.same_result(_device_rescore(hip, ix, q, qcu, cand, k), want), (n_cand, k)
    assert (ix.rescore(q, qcu, cand, 256)[0][:, 0] >= 0).all()
    # a repeated id counts as that many candidates; k may exceed n_cand
    got = ix.rescore(q[:qcu[1]], qcu[:2], [[7, 7, 2, 7]], 6)
    assert sorted(got[0][0].tolist()) == [-1, -1, 2, 7, 7, 7] and tref.same_result(got, tref.rescore_expected(S[:1], [[7, 7, 2, 7]], 6))
    # out-of-range ids: the host form refuses them, the device form skips them
    wild = cand[:, :33].copy()
    wild[:, 3], wild[:, 7], wild[:, 11] = N_DOCS, -7, 2 ** 31 - 1
    with pytest.raises(ValueError):
        ix.rescore(q, qcu, wild, 10)
    assert tref.same_result(_device_rescore(hip, ix, q, qcu, wild, 10), tref.rescore_expected(S, wild, 10))
    # a query longer than a search takes is rescored all the same (maxsim's kernel has no such limit)
    long_q = mr.unit_rows(rng, 200, 64)
    want = tref.rescore_expected(model.maxsim(long_q, [0, 200], c["d"], c["dcu"]), cand[:1, :33], 10)
    assert tref.same_result(ix.rescore(long_q, [0, 200], cand[:1, :33], 10), want)
    ix.close()


def test_a_dense_searchs_ids_feed_rescore_on_the_device(model):
    """BertIndex.search_device writes d_ids; rescore_device reads them on the same stream, with no host copy between"""
    c = _case(model, 64)
    q, qcu = c["q"], c["qcu"]
    nq = len(qcu) - 1
    hip = Hip()
    rng = np.random.default_rng(6)
    tix = _index(model, 64, c["d"], c["dcu"])
    dense = model.index(32, "f32")
    dense.add(mr.unit_rows(rng, N_DOCS, 32))
    dq = mr.unit_rows(rng, nq, 32)
    d_dq, d_cand, d_csc = hip.upload(dq), hip.nans((nq, 20), np.int32), hip.nans((nq, 20), np.float32)
    d_q, d_qcu = _f16(hip, q), hip.upload(qcu)
    d_ids, d_sc = hip.nans((nq, 10), np.int32), hip.nans((nq, 10), np.float32)
    s = hip.stream()
    dense.search_device(nq, d_dq, 20, d_cand, d_csc, s)
    tix.rescore_device(nq, d_qcu, d_q, 20, d_cand, 10, d_ids, d_sc, s)
    got = hip.download(d_ids, (nq, 10), np.int32), hip.download(d_sc, (nq, 10), np.float32)
    cand, _ = dense.search(dq, 20)
    assert (cand >= 0).all()
    want = tix.rescore(q, qcu, cand, 10)
    assert tref.same_result(got, want) and tref.same_result(want, tref.rescore_expected(c["S"], cand, 10))
    hip.destroy_stream(s)
    hip.free(d_dq, d_cand, d_csc, d_q, d_qcu, d_ids, d_sc)
    dense.close(); tix.close()


# ------------------------------------------------------------------------------------------------
# capture
# ------------------------------------------------------------------------------------------------
def test_search_and_rescore_are_captured_and_replayed(model):
    c = _case(model, 64)
    q, qcu = c["q"], c["qcu"]
    nq, k, n_cand = len(qcu) - 1, 10, 33
    hip = Hip()
    ix = model.token_index(64)
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
    assert tref.same_result(eager[:2], tref.search_expected(c["S"], k)) and tref.same_result(eager[2:], tref.rescore_expected(c["S"], cand, k))
    with hip.capture(s) as cap:
        ix.search_device(nq, d_qcu, d_q, 128, k, outs[0], outs[1], s)
        ix.rescore_device(nq, d_qcu, d_q, n_cand, d_c, k, outs[2], outs[3], s)
    assert cap.status == 0 and cap.graph and hip.kernel_nodes(cap.graph) == 5          # scan, merge; pairs, maxsim, merge
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
# launch geometry
# ------------------------------------------------------------------------------------------------
def test_two_hundred_thousand_one_token_documents(model):
    dim, n = 8, 200000
    rng = np.random.default_rng(12)
    d = mr.unit_rows(rng, n, dim)
    d[150001] = d[17]                            # a tie across distant slices
    dcu = np.arange(n + 1, dtype=np.int32)
    q, qcu = tref.queries(rng, dim, [33])
    S = model.maxsim(q, qcu, d, dcu)
    ix = _index(model, dim, d, dcu)
    assert pybert.test_token_index_plan(n, 1, 0)[0] > 1000
    for k in (10, 256):
        assert tref.same_result(ix.search(q, qcu, k), tref.search_expected(S, k)), k
    ix.close()


# ------------------------------------------------------------------------------------------------
# texts and the example
# ------------------------------------------------------------------------------------------------
LINES = ["hello world", "testing servers, clients!", "embedding test.", "pool index search row", "long text window", "a b c d e f g h i j a b c",
         "hello hello world world", "search row index", "text window stride long text", "", "a " * 80, "client server embedding pool"]
QUERIES = ["long text window stride", "hello", "index search"]


def test_texts_go_through_the_token_rows_pass(text_model):
    m = pybert.BertModel(text_model[0])
    m.set_option("chunk_tokens", "70")           # the lines are cut into several chunks
    ix = m.token_index()
    assert ix.add_texts(LINES[:5]) == 0 and ix.add_texts(LINES[5:]) == 5 and len(ix) == len(LINES)
    m.set_option("chunk_tokens", "262144")
    rows, cu = m.encode_tokens(LINES, normalize=True)
    assert ix.n_tokens() == int(cu[-1])
    for i in range(len(LINES)):
        want = rows[cu[i]:cu[i + 1]].astype(np.float16).astype(np.float32)
        assert np.array_equal(ix.get_doc(i).view(np.uint32), want.view(np.uint32)), i
    qrows, qcu = m.encode_tokens(QUERIES, normalize=True)
    want = ix.search(qrows, qcu, 5)
    assert tref.same_result(ix.search_texts(QUERIES, 5), want)
    assert tref.same_result(want, tref.search_expected(m.maxsim(qrows, qcu, rows, cu), 5))
    # another dim than the model's: the text routes refuse, the index unchanged
    other = m.token_index(ix.dim + 8)
    with pytest.raises(ValueError):
        other.add_texts(LINES)
    assert len(other) == 0
    other.close(); ix.close(); m.close()


def test_bert_search_token_index_and_late(text_model, tmp_path):
    path, _ = text_model
    lines = [l for l in LINES if l]
    f = tmp_path / "lines.txt"
    f.write_text("\n".join(lines) + "\n")
    exe = os.path.join(BIN, "bert-search")
    stdin = "".join(q + "\n" for q in QUERIES) + "q\n"
    run = lambda flags: subprocess.run([exe, "-m", path, "-f", str(f), "-k", "3"] + flags, input=stdin, capture_output=True, text=True, timeout=300)
    plain, kept = run(["--maxsim", "20"]), run(["--maxsim", "20", "--token-index"])
    assert plain.returncode == 0 and kept.returncode == 0, (plain.stderr, kept.stderr)
    assert plain.stdout.count("MaxSim score") == 3 * len(QUERIES) and kept.stdout == plain.stdout
    late = run(["--late"])
    assert late.returncode == 0, late.stderr
    m = pybert.BertModel(path)
    ix = m.token_index()
    ix.add_texts(lines)
    ids, sc = ix.search_texts(QUERIES, 3)
    prompt = "Enter a text to find similar texts (enter 'q' to quit): "
    want = f"Loading texts from {f}...\nLoaded {len(lines)} lines.\n"
    for i in range(len(QUERIES)):
        want += prompt + "\nClosest texts:\n" + "".join(f"{j + 1}. {lines[ids[i][j]]}\n (MaxSim score: {sc[i][j]:.4f})\n" for j in range(3))
    assert late.stdout == want + prompt + "\n"
    ix.close(); m.close()


def test_worst_fractions_are_recorded():
    """(last in the file) every float64 bound above was met: the figures, for the log"""
    for what, frac in sorted(_WORST.items()):
        print(f"{what}: {frac:.3f}")
    assert _WORST and all(f <= 1.0 for f in _WORST.values())
