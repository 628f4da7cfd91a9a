"""GPU tests of the sparse index's postings and inverted search (bert_hip.h "Sparse index: postings and the inverted search").  No
test has a tolerance: equality means equal ids and equal f32 bits.  The oracles are tests/sparse_index_reference.py and the index's
own row-major search / search_filtered on the same object.  Unless a test says otherwise the postings are built with
"sparse_index_segment_rows" = 256, so that 700 rows are three segments, the last one partial and ending inside a block of 64."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from bert_cpp_amd import ggml_file as gf
from bert_cpp_amd import pybert

import hip_graph
import sparse_index_reference as ref
import sparse_inverted_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
OK = hip_graph.HIP_SUCCESS
NQ, SEG, ROWS = cases.NQ, cases.SEG_TEST, cases.ROWS
KS = (1, 10, 256)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _p(a):
    return a.ctypes.data


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hook_model(make_model):
    """a context of libbert_test.so: the postings' read-back hook takes its indexes"""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path, test_routes=True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hip():
    return hip_graph.Hip()


def _segment_rows(model, seg):
    model.set_option("sparse_index_segment_rows", str(seg))


def _index(model, name, dtype, rows=None, seg=SEG, splits=None):
    """the case's rows in an index of model with postings in segments of seg rows (0 = the default)"""
    V, _, width = cases.CASES[name][:3]
    ids, w, _, _ = cases.data(name, rows)
    ix = model.sparse_index(width, dtype, n_vocab=V)
    for a, b in splits or ((0, len(ids)),):
        ix.add(ids[a:b], w[a:b])
    _segment_rows(model, seg)
    assert ix.invert() == len(ids) == ix.inverted_rows == len(ix)
    return ix


# ------------------------------------------------------------------------------------------------
# 1. search equals the reference and the row-major search
# ------------------------------------------------------------------------------------------------
SEARCH = [(n, d) for n, c in cases.CASES.items() for d in c[1]]


@pytest.mark.parametrize("name,dtype", SEARCH, ids=[f"{n}-{d}" for n, d in SEARCH])
def test_search_equals_the_reference_and_the_row_major_search(model, name, dtype):
    V, _, width, fill, rows, kq, qfill, skew = cases.CASES[name]
    seg = 0 if name == "c_default_seg" else SEG
    ids, w, q_ids, q_w = cases.data(name)
    sc = cases.scores(name, dtype)
    ix = _index(model, name, dtype, seg=seg)
    code = ("f32", "f16").index(dtype)
    g = pybert.test_sparse_postings_geometry(code, V, rows, NQ, 10, seg or cases.SEG_DEFAULT)
    if rows == ROWS:
        assert -(-rows // SEG) == 3 and rows % SEG % 64 != 0 and g["n_slices"] == 3, g
    if name == "c_default_seg":
        assert g["n_slices"] == 3 and rows % cases.SEG_DEFAULT == 130
    # (k) the query of only -1s: every row scores +0 and the smallest ids win; (l) the query whose terms no row has: the same
    assert (q_ids[0] == -1).all() and not sc[0].any()
    if V > 40:
        assert set(q_ids[4][q_ids[4] >= 0]) == set(cases.ABSENT) and not np.isin(ids, cases.ABSENT).any() and not sc[4].any()
    if name in ("e", "f", "g") or name.startswith("c"):
        assert (ids == V - 1).any() and (q_ids == V - 1).any() and sc[3, 3] != 0      # the vocabulary's last id, stored and queried
    if name == "d":
        assert (sc == 0).mean() > 0.9
    if name == "b":
        assert (sc != 0).mean() > 0.5
    for k in KS:
        want = cases.want(sc, k)
        got = ix.search_inverted(q_ids, q_w, k)
        assert _same(got, want), (name, dtype, k)
        assert _same(got, ix.search(q_ids, q_w, k)), (name, dtype, k)
        if k == 10 and rows >= 10:
            for q in (0, 4) if V > 40 else (0,):
                assert np.array_equal(got[0][q], np.arange(10)) and not _bits(got[1][q]).any()
    ix.close()


def test_an_empty_index_inverts_to_nothing_and_answers_with_empty_slots(model):
    ix = model.sparse_index(16, "f32", n_vocab=100)
    _segment_rows(model, SEG)
    assert ix.invert() == 0 and ix.inverted_rows == 0
    q_ids, q_w = np.array([[1, 2, -1]], np.int32), np.ones((1, 3), np.float32)
    for k in KS:
        got = ix.search_inverted(q_ids, q_w, k)
        assert (got[0] == -1).all() and np.isneginf(got[1]).all()
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("rows", [SEG - 1, SEG, SEG + 1])
def test_row_counts_around_a_segment(model, rows, dtype):
    _, _, q_ids, q_w = cases.data("a", rows)
    sc = cases.scores("a", dtype, rows)
    ix = _index(model, "a", dtype, rows)
    for k in KS:
        got = ix.search_inverted(q_ids, q_w, k)
        assert _same(got, cases.want(sc, k)) and _same(got, ix.search(q_ids, q_w, k)), (rows, k)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 2. the postings, read back
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("a", "f32"), ("a", "f16"), ("g", "f32")])
def test_the_postings_are_the_stored_rows_term_major(hook_model, name, dtype):
    V, _, width, _, rows = cases.CASES[name][:5]
    ix = _index(hook_model, name, dtype)
    st_i, st_w = ix.get_rows(np.arange(rows))
    n_segs = -(-rows // SEG)
    for sg in range(n_segs):
        off, prow, pw, seg_rows = pybert.test_sparse_postings_segment(ix, sg)
        assert seg_rows == SEG
        lo, hi = sg * SEG, min(rows, (sg + 1) * SEG)
        used = st_i[lo:hi] >= 0
        assert (np.diff(off.astype(np.int64)) >= 0).all() and off[0] == 0 and off[-1] == used.sum() == len(prow)
        assert (prow >= 0).all() and (prow < hi - lo).all()
        # every list, as a set of (local row, weight bits), is what the stored rows imply: compare all lists at once, each sorted
        r, c = np.nonzero(used)
        want = np.stack([st_i[lo:hi][r, c].astype(np.int64), r.astype(np.int64), _bits(st_w[lo:hi][r, c]).astype(np.int64)], 1)
        got_id = np.repeat(np.arange(V, dtype=np.int64), np.diff(off.astype(np.int64)))
        got = np.stack([got_id, prow.astype(np.int64), _bits(pw).astype(np.int64)], 1)
        order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
        assert np.array_equal(order(got), order(want)), (name, sg)
    with pytest.raises(RuntimeError):
        pybert.test_sparse_postings_segment(ix, n_segs)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 3. a score depends on its query and its row alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_result_depends_on_its_query_and_its_rows_alone(model, dtype):
    _, _, q_ids, q_w = cases.data("a")
    k = 10
    want = cases.want(cases.scores("a", dtype), k)
    ix = _index(model, "a", dtype)
    batch = ix.search_inverted(q_ids, q_w, k)
    assert _same(batch, want)
    for q in range(NQ):
        alone = ix.search_inverted(q_ids[q:q + 1], q_w[q:q + 1], k)
        assert _same(alone, (batch[0][q:q + 1], batch[1][q:q + 1])), q
    try:
        for qb in (1, 2, 8):
            model.set_option("sparse_index_qb", str(qb))
            assert _same(ix.search_inverted(q_ids, q_w, k), batch), qb
    finally:
        model.set_option("sparse_index_qb", "0")
    for seg in (1024, 0):
        _segment_rows(model, seg)
        assert ix.invert() == ROWS
        assert _same(ix.search_inverted(q_ids, q_w, k), batch), seg
        assert _same(ix.search_inverted(q_ids, q_w, 256), cases.want(cases.scores("a", dtype), 256)), seg
    ix.close()
    # postings built after adds of 1 + 62 + 637 rows
    parts = _index(model, "a", dtype, splits=((0, 1), (1, 63), (63, ROWS)))
    assert _same(parts.search_inverted(q_ids, q_w, k), batch)
    parts.close()


# ------------------------------------------------------------------------------------------------
# 4. removed rows and allow-lists
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_removed_rows_and_allow_lists_equal_search_filtered(model, dtype, capfd):
    _, _, q_ids, q_w = cases.data("a")
    sc = cases.scores("a", dtype)
    rng = np.random.default_rng(5)
    ix = _index(model, "a", dtype)
    allow = rng.random(ROWS) < 0.3
    none = np.zeros(ROWS, bool)
    one = none.copy()
    one[ROWS - 7] = True                                          # one row of the last, partial segment
    live = np.ones(ROWS, bool)

    def check(allowed, what):
        for k in KS:
            got = ix.search_inverted(q_ids, q_w, k, allow=allowed)
            q = live if allowed is None else live & allowed
            assert _same(got, cases.want(sc, k, q)), (what, k)
            assert _same(got, ix.search(q_ids, q_w, k, allow=allowed)), (what, k)

    check(allow, "an allow-list")
    check(none, "an allow-list with no bit set")
    check(one, "one row of the last segment")
    got = ix.search_inverted(q_ids, q_w, 10, allow=one)
    assert (got[0][:, 0] == ROWS - 7).all() and (got[0][:, 1:] == -1).all()
    gone = rng.permutation(ROWS)[:200]
    assert ix.remove(gone) == 200 and ix.inverted_rows == ROWS    # remove keeps the postings: no rebuild
    live[gone] = False
    check(None, "removed rows")
    check(allow, "removed rows and an allow-list")
    # too few words
    out_i, out_s = np.full((NQ, 4), 7, np.int32), np.full((NQ, 4), 7.0, np.float32)
    words = pybert.allow_words(allow, ROWS)
    capfd.readouterr()
    r = model.lib.bert_hip_sparse_index_search_inverted(ix.ix, NQ, q_ids.shape[1], _p(q_ids), _p(q_w), 4, _p(words), len(words) - 1, _p(out_i), _p(out_s))
    assert r == -2 and "words" in capfd.readouterr().err and (out_i == 7).all() and (out_s == 7.0).all()
    ix.close()


# ------------------------------------------------------------------------------------------------
# 5. life cycle
# ------------------------------------------------------------------------------------------------
def test_stale_and_missing_postings_are_refused_and_invert_restores_them(model, tmp_path, capfd):
    V, _, width = cases.CASES["a"][:3]
    ids, w, q_ids, q_w = cases.data("a")
    sc = cases.scores("a", "f16")
    k = 10
    _segment_rows(model, SEG)
    ix = model.sparse_index(width, "f16", n_vocab=V)
    ix.add(ids[:300], w[:300])
    out_i, out_s = np.full((NQ, k), 7, np.int32), np.full((NQ, k), 7.0, np.float32)

    def refused():
        capfd.readouterr()
        r = model.lib.bert_hip_sparse_index_search_inverted(ix.ix, NQ, q_ids.shape[1], _p(q_ids), _p(q_w), k, None, 0, _p(out_i), _p(out_s))
        err = capfd.readouterr().err
        assert r == -2 and "bert_hip_sparse_index_invert" in err, (r, err)
        assert (out_i == 7).all() and (out_s == 7.0).all()

    assert ix.inverted_rows == 0
    refused()                                                     # before invert
    assert ix.invert() == 300
    assert _same(ix.search_inverted(q_ids, q_w, k), cases.want(sc[:, :300], k))
    ix.add(ids[300:], w[300:])
    assert ix.inverted_rows == 300 and len(ix) == ROWS
    refused()                                                     # rows added since
    assert _same(ix.search(q_ids, q_w, k), cases.want(sc, k))     # (the row-major search does not care)
    assert ix.invert() == ROWS
    fresh = _index(model, "a", "f16")
    for kk in KS:
        assert _same(ix.search_inverted(q_ids, q_w, kk), fresh.search_inverted(q_ids, q_w, kk))
        assert _same(ix.search_inverted(q_ids, q_w, kk), cases.want(sc, kk))
    fresh.close()
    # compact: the ids change, the postings go
    gone = np.arange(0, ROWS, 3)
    ix.remove(gone)
    old = ix.compact()
    assert ix.inverted_rows == 0 and len(ix) == ROWS - len(gone) and np.array_equal(old, np.setdiff1d(np.arange(ROWS), gone))
    refused()
    assert ix.invert() == len(old)
    got = ix.search_inverted(q_ids, q_w, k)
    assert _same(got, cases.want(sc[:, old], k)) and _same(got, ix.search(q_ids, q_w, k))
    # a loaded index has no postings
    path = str(tmp_path / "rows.spx")
    ix.save(path)
    loaded = model.load_sparse_index(path)
    assert loaded.inverted_rows == 0
    with pytest.raises(ValueError):
        loaded.search_inverted(q_ids, q_w, k)
    assert loaded.invert() == len(old) and _same(loaded.search_inverted(q_ids, q_w, k), got)
    loaded.close()
    ix.close()


# ------------------------------------------------------------------------------------------------
# 6. host errors, device input
# ------------------------------------------------------------------------------------------------
def test_host_refusals_leave_the_outputs_untouched(model, capfd):
    L = model.lib
    V, width = 100, 8
    rng = np.random.default_rng(2)
    ids, w = cases._terms(rng, 70, width, V, width)
    ix = model.sparse_index(width, "f32", n_vocab=V)
    ix.add(ids, w)
    _segment_rows(model, SEG)
    ix.invert()
    out_i, out_s = np.full((2, 4), 7, np.int32), np.full((2, 4), 7.0, np.float32)
    good_i, good_w = np.array([[1, 5, -1, 9], [-1, -1, -1, -1]], np.int32), np.ones((2, 4), np.float32)

    def call(i, x, k=4, kq=4):
        capfd.readouterr()
        r = L.bert_hip_sparse_index_search_inverted(ix.ix, 2, kq, _p(i), _p(x), k, None, 0, _p(out_i), _p(out_s))
        return r, capfd.readouterr().err

    def refused(rc, what):
        r, err = rc
        assert r == -2 and what in err, (r, what, err)
        assert (out_i == 7).all() and (out_s == 7.0).all()

    for k in (0, 257):
        refused(call(good_i, good_w, k=k), "k must be")
    for kq in (0, 257):
        refused(call(good_i, good_w, kq=kq), "kq must be")
    bad = good_i.copy(); bad[1, 3] = V
    refused(call(bad, good_w), "outside")
    bad = good_i.copy(); bad[0, 3] = 5
    refused(call(bad, good_w), "twice")
    for x in (np.nan, np.inf):
        bw = good_w.copy(); bw[0, 1] = x
        refused(call(good_i, bw), "not finite")
    assert call(good_i, good_w)[0] == 0 and _same((out_i, out_s), ix.search(good_i, good_w, 4))
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_device_queries_count_bad_ids_as_unused_and_a_repeated_id_stays_in_its_query(model, hip, dtype):
    rng = np.random.default_rng(23)
    V, width, rows, kq, nq, k = 1000, 16, 300, 16, 9, 20
    ids, w = cases._terms(rng, rows, width, V, width, 2.0)
    q_ids, q_w = cases._terms(rng, nq, kq, V, kq, 2.0)
    flat = q_ids.reshape(-1)
    for j, bad in zip(rng.permutation(flat.size)[:40], np.resize([V, V + 1, -2, -7, 2 ** 31 - 1, -2 ** 31, 65536, 262144, 1 << 20], 40)):
        flat[j] = bad
    clean = np.where((q_ids >= 0) & (q_ids < V), q_ids, -1).astype(np.int32)
    st = ref.stored_rows(ids, w, width, dtype)
    want = ref.search(st[0], st[1], clean, q_w, V, k)
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.add(ids, w)
    _segment_rows(model, SEG)
    ix.invert()
    d_oi, d_os = hip.nans((nq, k), np.int32), hip.nans((nq, k))

    def run(qi):
        d_qi, d_qw = hip.upload(qi), hip.upload(q_w)
        ix.search_inverted_device(nq, kq, d_qi, d_qw, k, d_oi, d_os)
        hip.sync()
        out = hip.download(d_oi, (nq, k), np.int32), hip.download(d_os, (nq, k))
        hip.free(d_qi, d_qw)
        return out

    assert _same(run(q_ids), want)
    # query 2 holds one of its ids twice: its own scores are unspecified, every other query of the call is exact, and so is the next call
    twice = q_ids.copy()
    used = np.flatnonzero(clean[2] >= 0)
    assert len(used) >= 2
    twice[2, used[1]] = twice[2, used[0]]
    got = run(twice)
    others = np.arange(nq) != 2
    assert _same((got[0][others], got[1][others]), (want[0][others], want[1][others]))
    assert _same(run(q_ids), want)
    hip.free(d_oi, d_os)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 7. stream capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_search_inverted_device_captures_and_replays_with_changed_queries(model, hip, dtype):
    V, _, width, _, _, kq = cases.CASES["a"][:6]
    ids, w, q_ids, q_w = cases.data("a")
    nq, k = 9, 10
    allow = np.random.default_rng(3).random(ROWS) < 0.5
    words = pybert.allow_words(allow, ROWS)
    _segment_rows(model, SEG)
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.reserve(ROWS, nq, k)
    ix.add(ids, w)
    assert ix.invert() == ROWS
    d_qi, d_qw, d_al = hip.upload(q_ids[:nq]), hip.upload(q_w[:nq]), hip.upload(words)
    d_ids, d_sc = hip.nans((2 * nq, k), np.int32), hip.nans((2 * nq, k))
    s = hip.stream()
    first = []
    with hip.capture(s) as cap:
        first.append(model.lib.bert_hip_sparse_index_search_inverted_device(ix.ix, nq, kq, d_qi, d_qw, k, None, 0, d_ids, d_sc, s))
        first.append(model.lib.bert_hip_sparse_index_search_inverted_device(ix.ix, nq, kq, d_qi, d_qw, k, d_al, len(words), d_ids + 4 * nq * k, d_sc + 4 * nq * k, s))
    assert first == [0, 0] and cap.status == OK and cap.graph
    assert (hip.download(d_ids, (2 * nq, k), np.int32) == -1).all(), "capturing must run nothing"
    assert hip.kernel_nodes(cap.graph) == 6                      # twice: query sort, scan, merge
    ex = hip.instantiate(cap.graph)
    for launch, lo in enumerate((0, 20, 40)):
        qi, qw = q_ids[lo:lo + nq], q_w[lo:lo + nq]
        hip.write(d_qi, qi)
        hip.write(d_qw, qw)
        hip.poison(d_ids, (2 * nq, k), np.int32)
        hip.poison(d_sc, (2 * nq, k))
        hip.launch(ex, s)
        got = hip.download(d_ids, (2 * nq, k), np.int32), hip.download(d_sc, (2 * nq, k))
        assert _same((got[0][:nq], got[1][:nq]), ix.search_inverted(qi, qw, k)), launch
        assert _same((got[0][nq:], got[1][nq:]), ix.search_inverted(qi, qw, k, allow=allow)), launch
        assert _same((got[0][:nq], got[1][:nq]), ix.search(qi, qw, k)), launch
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(d_qi, d_qw, d_al, d_ids, d_sc)
    ix.close()


def test_a_capture_that_would_have_to_allocate_is_refused(model, hip, capfd):
    """No reserve: the inverted search has to size its workspace inside the capture, which fails as it does for the existing device
    forms (tests/test_gpu_stream_capture.py: -3 after hipMalloc's "operation not permitted when stream is capturing", no graph).  Run
    once; the stream of the broken capture is only destroyed.  The index is unharmed."""
    V, _, width, _, _, kq = cases.CASES["a"][:6]
    ids, w, q_ids, q_w = cases.data("a")
    nq, k = 9, 10
    _segment_rows(model, SEG)
    ix = model.sparse_index(width, "f32", n_vocab=V)
    ix.add(ids, w)
    assert ix.invert() == ROWS
    d_qi, d_qw = hip.upload(q_ids[:nq]), hip.upload(q_w[:nq])
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k))
    s = hip.stream()
    capfd.readouterr()
    with hip.capture(s) as cap:
        r = model.lib.bert_hip_sparse_index_search_inverted_device(ix.ix, nq, kq, d_qi, d_qw, k, None, 0, d_ids, d_sc, s)
    err = capfd.readouterr().err
    assert r == -3 and "captur" in err, (r, err)
    assert cap.status != OK or not cap.graph or hip.kernel_nodes(cap.graph) == 0
    assert (hip.download(d_ids, (nq, k), np.int32) == -1).all()
    assert _same(ix.search_inverted(q_ids, q_w, k), ix.search(q_ids, q_w, k))
    hip.destroy_stream(s)
    hip.free(d_qi, d_qw, d_ids, d_sc)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 8. texts and bert-search --sparse --inverted
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_model(model_dir, tok_golden):
    """tiny dims over the golden tokenizer's vocabulary, with the MLM head (the fixture of tests/test_gpu_sparse_index.py's text routes)"""
    n = tok_golden["n_vocab"]
    vocab = [f"[unused{i}]" for i in range(n)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    for i, p in tok_golden["sparse_vocab"].items():
        vocab[int(i)] = p
    hp = dataclasses.replace(gf.MODEL_DIMS["tiny"], n_vocab=n)
    path = os.path.join(model_dir, "sparse_inverted_text.bin")
    gf.write_model(path, hp, gf.synthetic_weights(hp, 11, mlm_head=True), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    return path, words


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_search_texts_inverted_equals_search_texts(text_model, dtype, capfd):
    path, words = text_model
    m = pybert.BertModel(path)
    rng = np.random.default_rng(4)
    texts = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 40, size=300)] + [""]
    queries = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 12, size=9)]
    width, kq, k = 48, 16, 10
    ix = m.sparse_index(width, dtype)
    ix.add_texts(texts)
    out_i, out_s = np.full((1, k), 7, np.int32), np.full((1, k), 7.0, np.float32)
    txt = (C.c_char_p * 1)(b"a")
    capfd.readouterr()
    assert m.lib.bert_hip_sparse_index_search_inverted_texts(ix.ix, 1, 1, txt, kq, k, _p(out_i), _p(out_s)) == -2
    assert "bert_hip_sparse_index_invert" in capfd.readouterr().err and (out_i == 7).all() and (out_s == 7.0).all()
    m.set_option("sparse_index_segment_rows", str(SEG))
    assert ix.invert() == len(texts)
    got = ix.search_texts_inverted(queries, kq, k)
    assert _same(got, ix.search_texts(queries, kq, k)) and (got[1] > 0).any()
    q_ids, q_w = m.encode_sparse(queries, kq)
    assert _same(got, ix.search_inverted(q_ids, q_w, k))
    ix.close()
    m.close()


def test_bert_search_sparse_inverted_prints_what_sparse_prints(text_model, tmp_path):
    path, words = text_model
    rng = np.random.default_rng(8)
    lines = [" ".join(rng.choice(words, size=int(n), replace=False)) for n in rng.integers(3, 12, size=10)]
    file = tmp_path / "lines.txt"
    file.write_text("\n".join(lines) + "\n")
    exe = os.path.join(BIN, "bert-search")
    runs = []
    for extra in ([], ["--inverted"]):
        r = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "16", "-k", "5"] + extra, input="\n".join(lines) + "\nq\n",
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        runs.append(r.stdout)
    assert runs[0] == runs[1] and runs[0].count("Closest texts:") == 10 and "similarity score" in runs[0]
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--hybrid", path, "--inverted"], input="q\n", capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--inverted" in r.stderr
