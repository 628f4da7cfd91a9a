"""The token index on ordered score sequences (topk_order_reference.py "token fixtures"): token_index_scan_kernel's candidate list at
its edges — a step that fills the list to slot L - 1 behind a stale threshold, the near miss, a sort at every step, slices that end
inside a step and inside a group of four waves —, the merge behind 17 slices, a rescore whose 1024 candidates carry the merge's own
exact fit, and calls of more queries than one internal chunk (TokenIndex::QCHUNK = 256).  test_topk_order_host.py proves on the CPU
that each fixture reaches its state.

Every score is one product by +-1, a max over equal values and sums of zeros, so the expected matrix is exact and nothing here has a
tolerance: ids and score bits must equal the order rule over that matrix (tor.reference_topk) and the host model of the kernel's walk
(tor.token_search), compared with token_index_reference.same_result."""
import numpy as np
import pytest

import token_index_reference as tref
import topk_order_reference as tor
from bert_cpp_amd import pybert
from hip_graph import Hip

from test_gpu_token_index import _device_rescore, _device_search, _index

pytestmark = pytest.mark.gpu

CHUNK = 256                              # TokenIndex::QCHUNK (token_index.h)


@pytest.fixture(scope="module")
def model(make_model):
    m = pybert.BertModel(make_model("tiny", "f16", 2)[0])
    yield m
    m.close()


def _expected(fx, kinds, k):
    """(the score matrix [nq, n] of the kinds, the order rule's result over it)"""
    S = np.stack([fx.scores[kk] for kk in kinds])
    return S, tor.reference_topk(S, True, k)


def _search_both(model, hip, ix, fx, k, slices, what):
    """search and search_device of every kind at every query length under the tuning key `slices`, against the order rule and the model
    of the walk that cut gives"""
    kinds, lens = tor.token_layout()
    q, qcu = tor.token_queries(kinds, lens)
    S, want = _expected(fx, kinds, k)
    n_slices, slice_docs = pybert.test_token_index_plan(fx.n, len(kinds), slices)
    walked = tor.token_search(S, k, n_slices, slice_docs)
    assert tref.same_result((walked["ids"], walked["scores"]), want), (what, "the model")
    model.set_option("token_index_slices", str(slices))
    try:
        got = ix.search(q, qcu, k)
        dev = _device_search(hip, ix, q, qcu, max(lens), k)
    finally:
        model.set_option("token_index_slices", "0")
    for name, res in (("search", got), ("search_device", dev)):
        for i, (kk, ln) in enumerate(zip(kinds, lens)):
            assert tref.same_result((res[0][i:i + 1], res[1][i:i + 1]), (want[0][i:i + 1], want[1][i:i + 1])), (what, name, kk, ln)
        assert tref.same_result(res, (walked["ids"], walked["scores"])), (what, name)


@pytest.mark.parametrize("k", tor.TOKEN_KS)
def test_search_on_ordered_and_exact_fit_sequences(model, k):
    """ascending, descending, constant, sawtooth, the staircase of this k and its near miss, each at query lengths 1 and 33: as one
    slice (25 steps, the last of 37 documents) and as planned (slices of 17 documents)"""
    fx = tor.token_fixture(k)
    hip = Hip()
    ix = _index(model, tor.TOKEN_DIM, fx.rows, fx.cu)
    for slices in (1, 0):
        _search_both(model, hip, ix, fx, k, slices, (k, slices))
    ix.close()


def test_search_over_seventeen_slices_and_two_merge_rounds(model):
    k = tor.TOKEN_MANY_K
    fx = tor.token_fixture(k, tor.TOKEN_MANY_DOCS)
    hip = Hip()
    ix = _index(model, tor.TOKEN_DIM, fx.rows, fx.cu)
    _search_both(model, hip, ix, fx, k, tor.TOKEN_MANY_SLICES, "17 slices")
    ix.close()


@pytest.mark.parametrize("k", [1, 129, 256])
def test_rescored_candidates_and_the_merge_s_exact_fit(model, k):
    """1024 candidates in the caller's order carry the merge's staircase and near miss (tor.merge_scores); then the same lists with
    repeated ids and -1 entries"""
    sc = tor.merge_scores(k)
    n = tor.MERGE_CAND
    per_doc = np.zeros((n, tor.TOKEN_DIM), np.float32)
    per_doc[:, 0], per_doc[:, 1] = sc["stair"], sc["over"]
    lens = np.array([tor.TOKEN_DOC_LENS[d % 5] for d in range(n)])
    rows, cu = np.repeat(per_doc, lens, axis=0), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    kinds = [kk for kk in tor.MERGE_KINDS for _ in tor.TOKEN_QUERY_LENS]
    qlens = [ln for _ in tor.MERGE_KINDS for ln in tor.TOKEN_QUERY_LENS]
    parts = []
    for kk, ln in zip(kinds, qlens):
        q = np.zeros((ln, tor.TOKEN_DIM), np.float32)
        col, sign = tor.MERGE_COLUMN[kk]
        if col >= 0:
            q[0, col] = sign
        parts.append(q)
    q, qcu = np.concatenate(parts), np.concatenate([[0], np.cumsum(qlens)]).astype(np.int32)
    S = np.stack([sc[kk] for kk in kinds])
    hip = Hip()
    ix = _index(model, tor.TOKEN_DIM, rows, cu)
    cand = np.tile(np.arange(n, dtype=np.int32), (len(kinds), 1))
    holes = cand.copy()
    holes[:, 5::97] = -1                                             # no candidate
    holes[:, 300:310] = holes[:, 290:300]                            # repeated ids, in one round of the merge and
    holes[:, 1000:1010] = holes[:, 20:30]                            # three rounds apart
    holes[0, 0] = -1
    for name, c in (("exact fit", cand), ("repeats and holes", holes)):
        want = tref.rescore_expected(S, c, k)
        m = tor.merge(np.where(c >= 0, np.take_along_axis(S, np.maximum(c, 0).astype(np.int64), axis=1), -np.inf).astype(np.float32),
                      np.where(c >= 0, c, tor.SENT).astype(np.int64), k)
        assert tref.same_result((m["ids"], m["scores"]), want), (k, name, "the model")
        if name == "exact fit":
            by = dict(zip(kinds, m["walks"]))
            assert by["stair"]["fit_stale"][0] and by["stair"]["max_slot"] == tor.MERGE_L - 1 and by["over"]["near_miss"][0]
        assert tref.same_result(ix.rescore(q, qcu, c, k), want), (k, name, "rescore")
        assert tref.same_result(_device_rescore(hip, ix, q, qcu, c, k), want), (k, name, "rescore_device")
    ix.close()


# ------------------------------------------------------------------------------------------------
# more queries than one internal chunk
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [CHUNK + 1, 2 * CHUNK + 1])
def test_calls_of_more_queries_than_a_chunk(model, nq):
    """one-token queries that cycle through the patterns: every row of search, search_device, rescore and rescore_device equals the
    same query served in a call of its own, and the order rule; a guarded (empty) query at position 256, the second chunk's first,
    gets empty slots in the device forms and leaves its neighbours"""
    k, n_cand = 10, 33
    fx = tor.token_fixture(k, 200)
    kinds = [tor.TOKEN_KINDS[i % len(tor.TOKEN_KINDS)] for i in range(nq)]
    q, qcu = tor.token_queries(kinds, [1] * nq)
    S, want = _expected(fx, kinds, k)
    cand = np.random.default_rng(nq).integers(-1, fx.n, (nq, n_cand)).astype(np.int32)         # -1 entries and repeated ids
    want_r = tref.rescore_expected(S, cand, k)
    hip = Hip()
    ix = _index(model, tor.TOKEN_DIM, fx.rows, fx.cu)
    alone = [ix.search(q[i:i + 1], [0, 1], k) for i in range(nq)]
    alone = np.concatenate([a[0] for a in alone]), np.concatenate([a[1] for a in alone])
    alone_r = [ix.rescore(q[i:i + 1], [0, 1], cand[i:i + 1], k) for i in range(nq)]
    alone_r = np.concatenate([a[0] for a in alone_r]), np.concatenate([a[1] for a in alone_r])
    assert tref.same_result(alone, want) and tref.same_result(alone_r, want_r)
    rows_equal = lambda got, ref: [i for i in range(nq) if not tref.same_result((got[0][i:i + 1], got[1][i:i + 1]), (ref[0][i:i + 1], ref[1][i:i + 1]))]
    for name, got, ref in (("search", ix.search(q, qcu, k), alone), ("search_device", _device_search(hip, ix, q, qcu, 1, k), alone),
                           ("rescore", ix.rescore(q, qcu, cand, k), alone_r), ("rescore_device", _device_rescore(hip, ix, q, qcu, cand, k), alone_r)):
        assert got[0].shape == (nq, k) and rows_equal(got, ref) == [], (nq, name)
    # the guard path at the chunk's offset: query 256 is empty, the rows behind it move up by one
    gcu = np.concatenate([qcu[:CHUNK + 1], qcu[CHUNK:-1]]).astype(np.int32)
    assert len(gcu) == nq + 1 and gcu[CHUNK + 1] == gcu[CHUNK] and (np.diff(np.delete(gcu, CHUNK + 1)) == 1).all() and gcu[-1] == nq - 1
    served = np.array([i if i < CHUNK else i - 1 for i in range(nq)])                           # the query row that position i scores
    served_kinds = [kinds[j] for j in served]
    Sg, want_g = _expected(fx, served_kinds, k)
    want_gr = tref.rescore_expected(Sg, cand, k)
    for name, got, ref in (("search_device", _device_search(hip, ix, q, gcu, 1, k), want_g), ("rescore_device", _device_rescore(hip, ix, q, gcu, cand, k), want_gr)):
        assert (got[0][CHUNK] == -1).all() and np.isneginf(got[1][CHUNK]).all(), (nq, name, "the guarded query")
        keep = np.arange(nq) != CHUNK
        assert tref.same_result((got[0][keep], got[1][keep]), (ref[0][keep], ref[1][keep])), (nq, name, "the neighbours")
    ix.close()
