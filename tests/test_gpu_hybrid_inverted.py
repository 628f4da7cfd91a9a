"""GPU tests of the hybrid search over the postings (include/bert_hip.h "Hybrid search", "Over the postings"):
bert_hip_dense_sparse_search_inverted[_device | _texts] return the ids and score bits of bert_hip_hybrid_search[...] on the same pair of
indexes.  No comparison has a tolerance: equality means equal ids and equal f32 bits.  The references are hybrid_reference.search over
D and S of the two stored forms — S from sparse_index_reference, D from index_reference (i8, b1; and f32 / f16 where the fixture's
scores are exact integers) or, for random f32 / f16 rows, whose MFMA chain is not restated in Python, the dense index's public rescore,
which is how the header defines D — and the row-major hybrid search on the same objects.  The cells and what each is there to reach
are tests/hybrid_inverted_cases.py's; tests/test_hybrid_inverted_host.py proves the reach from the library's own plan."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import hip_graph
import hybrid_inverted_cases as hic
import hybrid_reference as href
import index_reference as ixr
import sparse_inverted_cases as cases
import topk_order_reference as tor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
OK = hip_graph.HIP_SUCCESS
HOOKS = (pybert.test_hybrid_chunk, pybert.test_sparse_postings_geometry)
_D = {}


def _p(a):
    return a.ctypes.data


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32))


@pytest.fixture(scope="module")
def model(make_model):
    """any model: both indexes only need the context's device.  It profiles, so that the last test can show which kernels this file ran."""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    yield m
    m.set_option("sparse_index_segment_rows", "0")
    m.close()


@pytest.fixture(scope="module")
def hip():
    return hip_graph.Hip()


def _invert(model, six, seg):
    model.set_option("sparse_index_segment_rows", str(seg))
    assert six.invert() == len(six) == six.inverted_rows


def _random_pair(model, dd, sd, seg, splits=None):
    rows, _, ids, w, _, _ = hic.random_data()
    dix, six = model.index(hic.R_DIM, dd), model.sparse_index(hic.R_WIDTH, sd, n_vocab=hic.R_V)
    for a, b in splits or ((0, hic.R_ROWS),):
        dix.add(rows[a:b])
        six.add(ids[a:b], w[a:b])
    _invert(model, six, seg)
    return dix, six


def _random_dense_scores(model, dd):
    """D [33][700] of the random case: NumPy for i8 and b1; for f32 and f16 the dense index's public rescore, every row a candidate"""
    if dd not in _D:
        rows, queries = hic.random_data()[:2]
        if dd in ("i8", "b1"):
            D = ixr.exact_scores(queries, rows, dd)
        else:
            ix = model.index(hic.R_DIM, dd)
            ix.add(rows)
            D = np.full((len(queries), hic.R_ROWS), np.nan, np.float32)
            for c0 in range(0, hic.R_ROWS, 256):
                m = min(256, hic.R_ROWS - c0)
                cand = np.full((len(queries), 256), -1, np.int32)
                cand[:, :m] = np.arange(c0, c0 + m)
                ids, sc = ix.rescore(queries, cand, 256)
                for q in range(len(queries)):
                    ok = ids[q] >= 0
                    D[q, ids[q][ok]] = sc[q][ok]
            ix.close()
            assert not np.isnan(D).any()
        D.setflags(write=False)
        _D[dd] = D
    return _D[dd]


# ------------------------------------------------------------------------------------------------
# 1. random rows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", hic.R_SEGS)
@pytest.mark.parametrize("sd", hic.SPARSE)
@pytest.mark.parametrize("dd", hic.DENSE)
def test_random_rows_equal_the_reference_and_the_row_major_search(model, dd, sd, seg):
    _, queries, _, _, q_ids, q_w = hic.random_data()
    D, S = _random_dense_scores(model, dd), hic.random_sparse_scores(sd)
    wd, ws = hic.R_WEIGHTS
    for mode in hic.R_MODES:
        gone_d, gone_s, allow, qual = hic.random_mode(mode)
        dix, six = _random_pair(model, dd, sd, seg)
        if len(gone_d):
            assert dix.remove(gone_d) == len(gone_d)
        if len(gone_s):
            assert six.remove(gone_s) == len(gone_s) and six.inverted_rows == hic.R_ROWS       # the postings stay
        for nq in hic.R_NQS:
            hic.check_random_plan(hic.plan(*HOOKS, sd, hic.R_V, hic.R_ROWS, nq, 10, seg), seg, nq)
            q = (queries[:nq], q_ids[:nq], q_w[:nq])
            for k in hic.R_KS:
                got = dix.hybrid_search_inverted(six, *q, k, wd, ws, allow=allow)
                assert _same(got, href.search(D[:nq], S[:nq], qual, wd, ws, k)), (mode, nq, k)
                assert _same(got, dix.hybrid_search(six, *q, k, wd, ws, allow=allow)), (mode, nq, k)
                if k > qual.sum():
                    assert (got[0][:, qual.sum():] == -1).all() and np.isneginf(got[1][:, qual.sum():]).all()
        dix.close()
        six.close()


# ------------------------------------------------------------------------------------------------
# 2. ordered and exact-fit scores
# ------------------------------------------------------------------------------------------------
def _ordered_pair(model, fx, gone_dense=(), gone_sparse=()):
    dix = model.index(dim=fx.rows.shape[1], dtype=fx.dd)
    six = model.sparse_index(fx.width, fx.sd, n_vocab=tor.SPARSE_V)
    assert dix.add(fx.rows) == 0 and six.add(fx.term_ids, fx.term_w) == 0 and len(dix) == len(six) == fx.n
    if len(gone_dense):
        assert dix.remove(gone_dense) == len(gone_dense)
    if len(gone_sparse):
        assert six.remove(gone_sparse) == len(gone_sparse)
    return dix, six


def _run_layouts(dix, six, fx, k, seg, allow=None, qual=None, what=""):
    want = tor.hybrid_reference(fx, k, qual)
    for nq in hic.O_NQS[seg]:
        p = hic.plan(*HOOKS, fx.sd, tor.SPARSE_V, fx.n, nq, k, seg)
        hic.check_ordered_plan(p, seg, nq)
        for name, lay in tor.layouts(fx.kinds, fx.busy, fx.idle, nq, p[0][0][2]["qb"]).items():
            got = dix.hybrid_search_inverted(six, *tor.hybrid_queries(fx, lay), k, fx.w[0], fx.w[1], allow=allow)
            ixr.assert_same(got, tor.of_layout(want, lay), (fx.name, what, seg, nq, name))


@pytest.mark.parametrize("mode", tor.MODES)
@pytest.mark.parametrize("k", hic.O_KS)
@pytest.mark.parametrize("sd", hic.SPARSE)
def test_ordered_and_exact_fit_scores_in_one_segment_and_in_sixteen(model, sd, k, mode):
    """the split carrier — neither D nor S alone orders the rows as H does — under every weight pair: seg 4096 (one segment) and
    seg 256 (every step a segment edge; 609 queries: workgroups that walk three segments, a slice that is the partial segment)"""
    for w in tor.HYBRID_WEIGHTS:
        fx = tor.hybrid_split_fixture(sd, sd, k, mode, w)
        if mode == "removed":
            gone_d, gone_s, allow = tor.hybrid_removed_split(fx.ok, True)
            dix, six = _ordered_pair(model, fx, gone_d, gone_s)
        else:
            dix, six = _ordered_pair(model, fx)
            allow = fx.ok
        for seg in hic.O_SEGS:
            _invert(model, six, seg)
            _run_layouts(dix, six, fx, k, seg, allow=allow, what=mode)
            if mode == "allow":                                      # the near miss: one row more than fits
                _run_layouts(dix, six, fx, k, seg, allow=fx.ok1, qual=fx.ok1, what="near miss")
        dix.close()
        six.close()


# ------------------------------------------------------------------------------------------------
# 3. global row, chunk-local query
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(model):
    fx = tor.many_hybrid_fixture()
    dix, six = _ordered_pair(model, fx)
    _invert(model, six, 0)
    yield fx, dix, six
    dix.close()
    six.close()


@pytest.mark.parametrize("k", hic.M_KS)
def test_seventeen_slices_read_their_own_rows_dense_scores(model, many, k):
    """every slice but the first finds its rows' D beyond the first slice's floats of the query's line of the score matrix"""
    fx, dix, six = many
    want = tor.hybrid_reference(fx, k)
    assert want["asc"][0][0, 0] == fx.n - 1 and want["desc"][0][0].tolist() == list(range(k))
    for nq in hic.M_NQS:
        hic.check_many_plan(hic.plan(*HOOKS, "f32", tor.SPARSE_V, fx.n, nq, k, 0), nq)
        lay = tor.many_layout(nq)
        got = dix.hybrid_search_inverted(six, *tor.hybrid_queries(fx, lay), k)
        ixr.assert_same(got, tor.of_layout(want, lay), (fx.name, k, nq))
        ixr.assert_same(got, dix.hybrid_search(six, *tor.hybrid_queries(fx, lay), k), (fx.name, k, nq, "row-major"))


def test_chunks_of_two_queries_read_the_matrix_by_the_chunks_index(model, many):
    fx, dix, six = many
    k, nq = 10, hic.M_CHUNK_NQ
    hic.check_many_plan(hic.plan(*HOOKS, "f32", tor.SPARSE_V, fx.n, nq, k, 0, pref=hic.M_CHUNK), nq, hic.M_CHUNK)
    lay = tor.many_layout(nq)
    q = tor.hybrid_queries(fx, lay)
    whole = dix.hybrid_search_inverted(six, *q, k)
    ixr.assert_same(whole, tor.of_layout(tor.hybrid_reference(fx, k), lay), "one chunk")
    try:
        model.set_option("hybrid_chunk_queries", str(hic.M_CHUNK))
        chunked = dix.hybrid_search_inverted(six, *q, k)
    finally:
        model.set_option("hybrid_chunk_queries", "0")
    ixr.assert_same(chunked, whole, "chunks of 2, 2 and 1")


# ------------------------------------------------------------------------------------------------
# 4. independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dd, sd", [("f16", "f32"), ("i8", "f16")])
def test_a_result_depends_on_its_query_and_its_rows_alone(model, dd, sd):
    _, queries, _, _, q_ids, q_w = hic.random_data()
    nq, k = 33, 20
    wd, ws = hic.R_WEIGHTS
    D, S = _random_dense_scores(model, dd), hic.random_sparse_scores(sd)
    dix, six = _random_pair(model, dd, sd, cases.SEG_TEST)
    batch = dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, wd, ws)
    assert _same(batch, href.search(D, S, np.ones(hic.R_ROWS, bool), wd, ws, k))
    for q in range(nq):
        alone = dix.hybrid_search_inverted(six, queries[q:q + 1], q_ids[q:q + 1], q_w[q:q + 1], k, wd, ws)
        assert _same(alone, (batch[0][q:q + 1], batch[1][q:q + 1])), q
    try:
        for qb in (1, 2, 4):
            model.set_option("sparse_index_qb", str(qb))
            assert pybert.test_sparse_postings_geometry(hic.SPARSE.index(sd), hic.R_V, hic.R_ROWS, 32, k, cases.SEG_TEST, qb)["qb"] == qb
            assert _same(dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, wd, ws), batch), qb
    finally:
        model.set_option("sparse_index_qb", "0")
    for seg in (1024, 2048, 256):
        _invert(model, six, seg)
        assert _same(dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, wd, ws), batch), seg
    # the two plain searches: weights (1, 0) and (0, 1)
    got = dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, 1.0, 0.0)
    plain = dix.search(queries, k)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    got = dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, 0.0, 1.0)
    plain = six.search(q_ids, q_w, k)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    allow = hic.random_masks()[2]
    got = dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, 1.0, 0.0, allow=allow)
    assert np.array_equal(got[0], dix.search(queries, k, allow=allow)[0])
    got = dix.hybrid_search_inverted(six, queries, q_ids, q_w, k, 0.0, 1.0, allow=allow)
    assert np.array_equal(got[0], six.search(q_ids, q_w, k, allow=allow)[0])
    dix.close()
    six.close()
    # both indexes built by adds of 1 + 62 + 637 rows
    pdix, psix = _random_pair(model, dd, sd, cases.SEG_TEST, splits=((0, 1), (1, 63), (63, hic.R_ROWS)))
    assert _same(pdix.hybrid_search_inverted(psix, queries, q_ids, q_w, k, wd, ws), batch)
    pdix.close()
    psix.close()


# ------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------
def test_missing_and_stale_postings_unequal_sizes_and_infinite_weights_are_refused(model, hip, capfd):
    rows, queries, ids, w, q_ids, q_w = hic.random_data()
    nq, k = 5, 10
    q, qi, qw = (np.array(a[:nq]) for a in (queries, q_ids, q_w))
    D, S = _random_dense_scores(model, "f16"), hic.random_sparse_scores("f32")
    model.set_option("sparse_index_segment_rows", str(cases.SEG_TEST))
    dix, six = model.index(hic.R_DIM, "f16"), model.sparse_index(hic.R_WIDTH, "f32", n_vocab=hic.R_V)
    dix.add(rows[:300])
    six.add(ids[:300], w[:300])
    out_i, out_s = np.full((nq, k), 7, np.int32), np.full((nq, k), 7.0, np.float32)
    d = [hip.upload(a) for a in (q, qi, qw)]
    d_i, d_s = hip.nans((nq, k), np.int32), hip.nans((nq, k))
    L = model.lib

    def host(wd=1.0, ws=1.0):
        return L.bert_hip_dense_sparse_search_inverted(dix.ix, six.ix, nq, _p(q), hic.R_KQ, _p(qi), _p(qw), wd, ws, None, 0, k, _p(out_i), _p(out_s))

    def device(wd=1.0, ws=1.0):
        return L.bert_hip_dense_sparse_search_inverted_device(dix.ix, six.ix, nq, d[0], hic.R_KQ, d[1], d[2], wd, ws, None, 0, k, d_i, d_s, None)

    def refused(what):
        for call in (host, device):
            capfd.readouterr()
            r = call()
            err = capfd.readouterr().err
            assert r == -2 and what in err, (call.__name__, r, err)
        assert (out_i == 7).all() and (out_s == 7.0).all() and (hip.download(d_i, (nq, k), np.int32) == -1).all()

    def answers(n, qual=None):
        want = href.search(D[:nq, :n], S[:nq, :n], np.ones(n, bool) if qual is None else qual, 1.0, 1.0, k)
        assert _same(dix.hybrid_search_inverted(six, q, qi, qw, k), want)
        assert device() == 0
        hip.sync()
        assert _same((hip.download(d_i, (nq, k), np.int32), hip.download(d_s, (nq, k))), want)
        hip.poison(d_i, (nq, k), np.int32)

    refused("bert_hip_sparse_index_invert")                         # before invert
    assert _same(dix.hybrid_search(six, q, qi, qw, k), href.search(D[:nq, :300], S[:nq, :300], np.ones(300, bool), 1.0, 1.0, k))
    assert six.invert() == 300
    answers(300)
    dix.add(rows[300:])
    six.add(ids[300:], w[300:])
    assert six.inverted_rows == 300 and len(six) == len(dix) == hic.R_ROWS
    refused("bert_hip_sparse_index_invert")                         # rows added to both indexes since
    with pytest.raises(ValueError):
        dix.hybrid_search_inverted(six, q, qi, qw, k)
    assert six.invert() == hic.R_ROWS
    answers(hic.R_ROWS)
    # remove on either side keeps the postings: no new invert
    gone_d, gone_s, _ = hic.random_masks()
    live = np.ones(hic.R_ROWS, bool)
    dix.remove(gone_d)
    live[gone_d] = False
    answers(hic.R_ROWS, live)
    six.remove(gone_s)
    live[gone_s] = False
    assert six.inverted_rows == hic.R_ROWS
    answers(hic.R_ROWS, live)
    # weights that are not finite
    for wd, ws in ((np.inf, 1.0), (1.0, -np.inf), (np.nan, 1.0)):
        for call in (host, device):
            capfd.readouterr()
            assert call(wd, ws) == -2 and "finite" in capfd.readouterr().err
    assert (out_i == 7).all() and (out_s == 7.0).all() and (hip.download(d_i, (nq, k), np.int32) == -1).all()
    # unequal sizes (the postings still cover the sparse index)
    extra = dix.add(rows[:1])
    assert extra == hic.R_ROWS and len(dix) == len(six) + 1
    refused("rows")
    six.add(ids[:1], w[:1])
    # compact drops the postings (the same rows removed on both sides first, so that the sizes agree afterwards)
    six.remove(np.concatenate([gone_d, [hic.R_ROWS]]).astype(np.int32))
    dix.remove(np.concatenate([gone_s, [hic.R_ROWS]]).astype(np.int32))
    old_s, old_d = six.compact(), dix.compact()
    assert six.inverted_rows == 0 and len(six) == len(dix) == int(live.sum()) and np.array_equal(old_s, old_d)
    refused("bert_hip_sparse_index_invert")
    assert six.invert() == len(six)
    want = href.search(D[:nq][:, old_s], S[:nq][:, old_s], np.ones(len(old_s), bool), 1.0, 1.0, k)
    assert _same(dix.hybrid_search_inverted(six, q, qi, qw, k), want)
    hip.free(*d, d_i, d_s)
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 6. capture and replay
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["reserve, invert", "invert, reserve"])
@pytest.mark.parametrize("dd, sd, masked", [("f16", "f32", False), ("i8", "f16", True)])
def test_a_reserved_and_inverted_device_call_is_captured_and_replayed(model, hip, dd, sd, masked, order):
    rows, queries, ids, w, q_ids, q_w = hic.random_data()
    nq, k = 9, 10
    wd, ws = hic.R_WEIGHTS
    model.set_option("sparse_index_segment_rows", str(cases.SEG_TEST))
    dix, six = model.index(hic.R_DIM, dd), model.sparse_index(hic.R_WIDTH, sd, n_vocab=hic.R_V)
    if order == "reserve, invert":
        dix.hybrid_reserve(six, hic.R_ROWS, nq, k)
    dix.add(rows)
    six.add(ids, w)
    assert six.invert() == hic.R_ROWS
    if order == "invert, reserve":
        dix.hybrid_reserve(six, hic.R_ROWS, nq, k)
    qual, words = np.ones(hic.R_ROWS, bool), None
    if masked:
        gone_d, gone_s, allow = hic.random_masks()
        dix.remove(gone_d)
        six.remove(gone_s)
        qual[gone_d] = False
        qual[gone_s] = False
        qual &= allow
        words = pybert.allow_words(allow, hic.R_ROWS)
    d_q, d_qi, d_qw = hip.upload(np.array(queries[:nq])), hip.upload(np.array(q_ids[:nq])), hip.upload(np.array(q_w[:nq]))
    d_allow = hip.upload(words) if masked else 0
    d_i, d_s = hip.nans((nq, k), np.int32), hip.nans((nq, k))
    s = hip.stream()
    call = lambda stream: model.lib.bert_hip_dense_sparse_search_inverted_device(dix.ix, six.ix, nq, d_q, hic.R_KQ, d_qi, d_qw, wd, ws, d_allow or None,
                                                                                 len(words) if masked else 0, k, d_i, d_s, stream)
    model.profile(False)                                            # (a timed launch cannot be captured)
    try:
        with hip.capture(s) as cap:
            r = call(s)
    finally:
        model.profile(True)
    assert r == 0 and cap.status == OK and cap.graph
    assert (hip.download(d_i, (nq, k), np.int32) == -1).all(), "capturing must run nothing"
    # the dense queries' ingest, scores, query sort, hybrid scan over the postings, merge — and the bitmap's AND in front
    assert hip.kernel_nodes(cap.graph) == 5 + int(masked)
    ex = hip.instantiate(cap.graph)
    D, S = _random_dense_scores(model, dd), hic.random_sparse_scores(sd)
    for step, lo in enumerate((0, 12)):
        hip.write(d_q, np.array(queries[lo:lo + nq]))
        hip.write(d_qi, np.array(q_ids[lo:lo + nq]))
        hip.write(d_qw, np.array(q_w[lo:lo + nq]))
        replays = []
        for _ in range(2):
            hip.poison(d_i, (nq, k), np.int32)
            hip.poison(d_s, (nq, k))
            hip.launch(ex, s)
            replays.append((hip.download(d_i, (nq, k), np.int32), hip.download(d_s, (nq, k))))
        hip.poison(d_i, (nq, k), np.int32)
        assert call(None) == 0
        eager = hip.download(d_i, (nq, k), np.int32), hip.download(d_s, (nq, k))
        assert _same(replays[0], eager) and _same(replays[1], eager), step
        assert _same(eager, href.search(D[lo:lo + nq], S[lo:lo + nq], qual, wd, ws, k)), step
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_q, d_qi, d_qw, d_i, d_s, *([d_allow] if masked else []))
    dix.close()
    six.close()


# ------------------------------------------------------------------------------------------------
# 7. the text route and bert-search
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_model(model_dir, tok_golden):
    """tiny dims over the golden tokenizer's vocabulary, with the MLM head (the fixture of tests/test_gpu_hybrid_search.py's text route)"""
    n = tok_golden["n_vocab"]
    vocab = [f"[unused{i}]" for i in range(n)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    for i, p in tok_golden["sparse_vocab"].items():
        vocab[int(i)] = p
    hp = dataclasses.replace(gf.MODEL_DIMS["tiny"], n_vocab=n)
    path = os.path.join(model_dir, "hybrid_inverted_text.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 11, mlm_head=True), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    return path, words


@pytest.mark.parametrize("dd, sd", [("f16", "f32"), ("i8", "f16")])
def test_the_text_route_equals_the_row_major_text_route(text_model, dd, sd, capfd):
    path, words = text_model
    m = pybert.BertModel(path)
    rng = np.random.default_rng(4)
    texts = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 40, size=300)]
    queries = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 12, size=9)]
    width, kq, k = 48, 16, 10
    dix, six = m.index(dtype=dd), m.sparse_index(width, sd)
    assert dix.add_texts(texts) == 0 and six.add_texts(texts) == 0
    out_i, out_s = np.full((1, k), 7, np.int32), np.full((1, k), 7.0, np.float32)
    txt = (C.c_char_p * 1)(b"a")
    capfd.readouterr()
    assert m.lib.bert_hip_dense_sparse_search_inverted_texts(dix.ix, six.ix, 1, 1, txt, kq, 1.0, 1.0, k, _p(out_i), _p(out_s)) == -2
    assert "bert_hip_sparse_index_invert" in capfd.readouterr().err and (out_i == 7).all() and (out_s == 7.0).all()
    m.set_option("sparse_index_segment_rows", str(cases.SEG_TEST))
    assert six.invert() == len(texts)
    for wd, ws in ((1.0, 1.0), (0.3, 0.01)):
        got = dix.hybrid_search_inverted_texts(six, queries, kq, k, wd, ws)
        assert _same(got, dix.hybrid_search_texts(six, queries, kq, k, wd, ws)) and (got[0] >= 0).all(), (wd, ws)
    q_ids, q_w = m.encode_sparse(queries, kq)
    assert _same(got, dix.hybrid_search_inverted(six, m.encode_batch(queries), q_ids, q_w, k, 0.3, 0.01))
    dix.close()
    six.close()
    m.close()


def test_bert_search_hybrid_postings_prints_what_hybrid_prints(text_model, tmp_path):
    path, words = text_model
    rng = np.random.default_rng(8)
    lines = [" ".join(rng.choice(words, size=int(n), replace=False)) for n in rng.integers(3, 12, size=10)]
    file = tmp_path / "lines.txt"
    file.write_text("\n".join(lines) + "\n")
    exe = os.path.join(BIN, "bert-search")
    base = [exe, "-m", path, "-f", str(file), "--hybrid", path, "--sparse-width", "16", "--weights", "0.5,0.25", "-k", "5"]
    runs = []
    for extra in ([], ["--postings"]):
        r = subprocess.run(base + extra, input="\n".join(lines) + "\nq\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs.append(r.stdout)
    assert runs[0] == runs[1] and runs[0].count("Closest texts:") == 10 and "similarity score" in runs[0]
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--postings"], input="q\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--postings" in r.stderr and "--hybrid" in r.stderr
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "16", "--postings"], input="q\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--postings" in r.stderr


# ------------------------------------------------------------------------------------------------
# 8. which kernels this file ran
# ------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_new_route_ran_under_this_file(model):
    """a small search per instantiation of its own (so that the test stands alone), then the profiler's launch counts"""
    _, queries, _, _, q_ids, q_w = hic.random_data()
    allow = hic.random_masks()[2]
    for dd, sd in zip(hic.DENSE, hic.SPARSE * 2):
        dix, six = _random_pair(model, dd, sd, cases.SEG_TEST)
        for al in (None, allow):
            assert _same(dix.hybrid_search_inverted(six, queries, q_ids, q_w, 10, allow=al), dix.hybrid_search(six, queries, q_ids, q_w, 10, allow=al))
        dix.close()
        six.close()
    rep = model.profile_report()
    names = [f"sparse_postings_hybrid_scan_{d}{m}" for d in hic.SPARSE for m in ("", "_masked")]
    names += [f"index_scores_{d}{m}" for d in hic.DENSE for m in ("", "_masked")] + ["sparse_query_sort", "mask_and", "topk_merge"]
    for name in names:
        print(f"{name}: {rep.get(name, {}).get('launches', 0)} launches")
    for name in names:
        assert rep.get(name, {}).get("launches", 0) >= 1, (name, sorted(rep))
