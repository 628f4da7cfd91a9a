"""GPU tests of the sparse index (bert_hip.h "Sparse index"): stored rows, search results, determinism, errors, hostile device input,
the text routes, stream capture and bert-search --sparse, all against tests/sparse_index_reference.py.  The reference is exact, the
operands are random: equality means bits, in ids and in scores, and the reference alone decides which rows come back."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bert.cpp_amd", "bin")
OK = hip_graph.HIP_SUCCESS
DTYPES = ["f32", "f16"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """(ids, scores or weights) pairs: equal ids, equal bits"""
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _p(a):
    return a.ctypes.data


@pytest.fixture(scope="module")
def model(make_model):
    """any model: a sparse index only needs the context's device"""
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def hip():
    return hip_graph.Hip()


def _weights(rng, shape):
    """f32 weights of both signs over twelve orders of magnitude"""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(np.float32)


def _terms(rng, n, kk, V, fill, skew=1.0):
    """n entries of kk columns: per entry up to fill distinct ids of [0, V) (drawn towards 0 for skew > 1, so entries share ids) at random
    places, -1 everywhere else; entry 0 has no term, entry 1 one, entry 2 as many as fit."""
    ids = np.full((n, kk), -1, np.int32)
    w = _weights(rng, (n, kk))
    top = min(fill, kk, V)
    for r in range(n):
        c = [0, 1, top][r] if r < 3 else int(rng.integers(0, top + 1))
        draw = np.unique((V * rng.random(4 * c + 8) ** skew).astype(np.int64))
        c = min(c, len(draw))
        ids[r, rng.permutation(kk)[:c]] = rng.permutation(draw)[:c]
    return ids, w


# ------------------------------------------------------------------------------------------------
# 1. add / get_rows
# ------------------------------------------------------------------------------------------------
F16_EDGES = np.array([2049.0, 2051.0, 2049.5, 2050.9, -2049.0, -2050.9, 1e-8, 65504.0, 0.0], np.float32)   # ties, up, down, underflow, largest


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [1, 5, 128, 256])
def test_add_get_rows_round_trip(model, width, dtype):
    rng = np.random.default_rng(width)
    V = 1000
    ids, w = _terms(rng, 130, width, V, width)
    used = np.argwhere(ids >= 0)
    for i, (r, c) in enumerate(used[:: max(1, len(used) // 40)]):
        w[r, c] = F16_EDGES[i % len(F16_EDGES)]
    # one row in the input order the MLM head writes: descending by weight, the unused places last
    full = ids[2] >= 0
    order = np.argsort(-w[2][full], kind="stable")
    ids[2], w[2] = np.concatenate([ids[2][full][order], ids[2][~full]]), np.concatenate([w[2][full][order], w[2][~full]])
    want = ref.stored_rows(ids, w, width, dtype)
    assert (want[0][0] == -1).all() and (want[0][1] >= 0).sum() == 1 and (want[0][2] >= 0).sum() == min(width, V)
    if dtype == "f16":
        assert not np.array_equal(_bits(want[1]), _bits(ref.stored_rows(ids, w, width, "f32")[1]))
    # adds of 1 + 62 + 67 rows start and end inside a block of 64
    ix = model.sparse_index(width, dtype, n_vocab=V)
    assert [ix.add(ids[a:b], w[a:b]) for a, b in ((0, 1), (1, 63), (63, 130))] == [0, 1, 63] and len(ix) == 130
    assert _same(ix.get_rows(np.arange(130)), want)
    pick = np.array([129, 0, 64, 63, 64, 2], np.int32)
    assert _same(ix.get_rows(pick), (want[0][pick], want[1][pick]))
    ix.close()
    for n in (1, 63, 64, 65, 130):
        ix = model.sparse_index(width, dtype, n_vocab=V)
        assert ix.add(ids[:n], w[:n]) == 0 and len(ix) == n
        assert _same(ix.get_rows(np.arange(n)), (want[0][:n], want[1][:n])), n
        ix.close()
    if width >= 5:
        # fewer columns than the index is wide
        ix = model.sparse_index(width, dtype, n_vocab=V)
        ids3, w3 = _terms(rng, 65, 3, V, 3)
        ix.add(ids3, w3)
        assert _same(ix.get_rows(np.arange(65)), ref.stored_rows(ids3, w3, width, dtype))
        ix.close()


# ------------------------------------------------------------------------------------------------
# 2. search against the reference
# ------------------------------------------------------------------------------------------------
NQ = 70
# (name, V, dtype, width, row fill, rows, kq, query fill, skew)
SEARCH_CASES = [
    ("small V, wide rows: most terms match", 40, "f32", 40, 40, 65, 256, 40, 1.0),
    ("one row, one query column", 40, "f16", 16, 16, 1, 1, 1, 1.0),
    ("V 1000", 1000, "f16", 128, 128, 1000, 32, 32, 2.0),
    ("large V, narrow rows: most rows score +0, ties by id", 30522, "f32", 5, 5, 5000, 32, 32, 1.0),
    ("V 30522, two slices", 30522, "f16", 128, 100, 5000, 256, 200, 3.0),
    ("V 65536, the largest u16 id", 65536, "f16", 64, 64, 64, 32, 32, 2.0),
    ("V 65537", 65537, "f32", 32, 32, 130, 32, 32, 2.0),
    ("V 262144, the largest query image", 262144, "f32", 256, 256, 130, 256, 256, 3.0),
]
_SEARCH = {}


def build_search_case(model, case):
    """index, queries and the reference's scores [NQ][rows] of a case, on model (other test files build their own: an index goes with
    its model)"""
    name, V, dtype, width, fill, rows, kq, qfill, skew = case
    rng = np.random.default_rng(len(name) + V)
    ids, w = _terms(rng, max(rows, 3), width, V, fill, skew)
    ids, w = ids[-rows:], w[-rows:]                              # (a single row: the full one)
    q_ids, q_w = _terms(rng, NQ, kq, V, qfill, skew)            # (query 0: only -1s)
    if rows > 3 and width > 1:
        ids[3], q_ids[3] = -1, -1                                # the vocabulary's last id, stored and asked for
        ids[3, :2], q_ids[3, 0] = [V - 1, 0], V - 1
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.add(ids, w)
    st = ref.stored_rows(ids, w, width, dtype)
    return ix, q_ids, q_w, ref.scores(st[0], st[1], q_ids, q_w, V)


def _search_case(model, case):
    """build_search_case, built once"""
    if case[0] not in _SEARCH:
        _SEARCH[case[0]] = build_search_case(model, case)
    return _SEARCH[case[0]]


@pytest.mark.parametrize("case", SEARCH_CASES, ids=[c[0] for c in SEARCH_CASES])
def test_search_equals_the_reference(model, case):
    name, V, dtype, width, fill, rows, kq, qfill, skew = case
    ix, q_ids, q_w, sc = _search_case(model, case)
    code = DTYPES.index(dtype)
    assert (q_ids[0] == -1).all() and not sc[0].any()            # the empty query: every row +0, the smallest ids win
    assert (sc < 0).any() or rows == 1
    if "most rows score +0" in name:
        assert (sc == 0).mean() > 0.9
    if "most terms match" in name:
        assert (sc != 0).mean() > 0.5
    for k in (1, 10, 256):
        g = pybert.test_sparse_scan_geometry(code, V, rows, NQ, k)
        if rows == 5000:
            # more than one slice, the last one ragged
            assert g["n_slices"] > 1 and rows % g["slice_rows"] != 0, g
        want = [ref.topk(s, k) for s in sc]
        want = np.stack([x[0] for x in want]), np.stack([x[1] for x in want])
        if k > rows:
            assert (want[0][:, rows:] == -1).all() and np.isneginf(want[1][:, rows:]).all()
        for nq in sorted({1, 2, g["qb"] - 1, g["qb"], g["qb"] + 1, NQ} - {0}):
            got = ix.search(q_ids[:nq], q_w[:nq], k)
            assert _same(got, (want[0][:nq], want[1][:nq])), (name, k, nq)


def test_empty_index(model):
    ix = model.sparse_index(8, "f32", n_vocab=100)
    ids, sc = ix.search(np.array([[3, -1]], np.int32), np.ones((1, 2), np.float32), 4)
    assert (ids == -1).all() and np.isneginf(sc).all() and len(ix) == 0
    assert ix.search(np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32), 4)[0].shape == (0, 4)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 3. determinism
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_result_depends_on_its_query_and_its_rows_alone(model, hip, dtype):
    rng = np.random.default_rng(17)
    V, width, rows, kq = 1000, 64, 3000, 32
    ids, w = _terms(rng, rows, width, V, width, 2.0)
    q_ids, q_w = _terms(rng, NQ, kq, V, kq, 2.0)
    probe = (q_ids[5:6].copy(), q_w[5:6].copy())
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.add(ids, w)
    alone = ix.search(*probe, 100)
    st = ref.stored_rows(ids, w, width, dtype)
    assert _same(alone, ref.search(st[0], st[1], *probe, V, 100))
    assert len(set(alone[1][0].tolist())) > 50                   # (not a trivial list)
    # at every position of a batch of 70
    for pos in range(NQ):
        b_ids, b_w = q_ids.copy(), q_w.copy()
        b_ids[pos], b_w[pos] = probe[0][0], probe[1][0]
        got = ix.search(b_ids, b_w, 100)
        assert _same((got[0][pos:pos + 1], got[1][pos:pos + 1]), alone), pos
    # k = 10 is the first 10 of k = 100; run to run
    top10 = ix.search(*probe, 10)
    assert _same(top10, (alone[0][:, :10], alone[1][:, :10]))
    assert _same(ix.search(*probe, 100), alone)
    # grown storage (three adds, no reserve) and reserved storage hold the same rows and answer alike
    grown, reserved = model.sparse_index(width, dtype, n_vocab=V), model.sparse_index(width, dtype, n_vocab=V)
    for a in range(0, rows, 1100):
        grown.add(ids[a:a + 1100], w[a:a + 1100])
    reserved.reserve(rows + 500, NQ, 100)
    reserved.add(ids[:1], w[:1])
    reserved.add(ids[1:], w[1:])
    for other in (grown, reserved):
        assert _same(other.get_rows(np.arange(rows)), st) and _same(other.search(*probe, 100), alone)
    # the device entry point
    d_qi, d_qw = hip.upload(probe[0]), hip.upload(probe[1])
    d_ids, d_sc = hip.nans((1, 100), np.int32), hip.nans((1, 100))
    reserved.search_device(1, kq, d_qi, d_qw, 100, d_ids, d_sc)
    assert _same((hip.download(d_ids, (1, 100), np.int32), hip.download(d_sc, (1, 100))), alone)
    hip.free(d_qi, d_qw, d_ids, d_sc)
    for x in (ix, grown, reserved):
        x.close()


# ------------------------------------------------------------------------------------------------
# 4. errors
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_leave_index_and_outputs_untouched(model, dtype, capfd):
    L = model.lib
    V, width = 100, 8
    rng = np.random.default_rng(2)
    ids, w = _terms(rng, 70, width, V, width)
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.add(ids, w)
    before = ix.get_rows(np.arange(70))
    out_i, out_s = np.full((2, 4), 7, np.int32), np.full((2, 4), 7.0, np.float32)
    capfd.readouterr()

    def refused(r, what):
        err = capfd.readouterr().err
        assert r == -2 and what in err, (r, what, err)
        assert len(ix) == 70 and (out_i == 7).all() and (out_s == 7.0).all()

    good_i, good_w = np.array([[1, 5, -1, 9], [-1, -1, -1, -1]], np.int32), np.ones((2, 4), np.float32)

    def bad(pos, id=None, weight=None):
        i, x = good_i.copy(), good_w.copy()
        if id is not None:
            i[pos] = id
        if weight is not None:
            x[pos] = weight
        return i, x

    cases = [(bad((0, 1), id=-2), "outside"), (bad((1, 3), id=V), "outside"), (bad((0, 3), id=5), "twice"),
             (bad((0, 0), weight=np.nan), "not finite"), (bad((0, 1), weight=np.inf), "not finite"), (bad((0, 3), weight=-np.inf), "not finite")]
    for (i, x), what in cases:
        refused(L.bert_hip_sparse_index_add(ix.ix, 2, 4, _p(i), _p(x)), what)
        refused(L.bert_hip_sparse_index_search(ix.ix, 2, 4, _p(i), _p(x), 4, _p(out_i), _p(out_s)), what)
    # a non-finite weight in an UNUSED place is ignored, as is a repeated -1
    i, x = bad((0, 2), weight=np.nan)
    assert L.bert_hip_sparse_index_search(ix.ix, 2, 4, _p(i), _p(x), 4, _p(out_i), _p(out_s)) == 0
    out_i[:], out_s[:] = 7, 7.0
    # 70000 is finite as f32 and infinite as f16: an f16 index refuses the row, an f32 index takes it; a query is never rounded
    i, x = bad((0, 0), weight=70000.0)
    if dtype == "f16":
        refused(L.bert_hip_sparse_index_add(ix.ix, 2, 4, _p(i), _p(x)), "not finite as f16")
    assert L.bert_hip_sparse_index_search(ix.ix, 2, 4, _p(i), _p(x), 4, _p(out_i), _p(out_s)) == 0
    out_i[:], out_s[:] = 7, 7.0
    # shapes
    wide_i, wide_w = np.full((1, width + 1), -1, np.int32), np.zeros((1, width + 1), np.float32)
    refused(L.bert_hip_sparse_index_add(ix.ix, 1, width + 1, _p(wide_i), _p(wide_w)), "k_in")
    refused(L.bert_hip_sparse_index_add(ix.ix, 1, 0, _p(wide_i), _p(wide_w)), "k_in")
    refused(L.bert_hip_sparse_index_add_device(ix.ix, 1, width + 1, None, None, None), "k_in")
    for k in (0, -1, 257):
        refused(L.bert_hip_sparse_index_search(ix.ix, 2, 4, _p(good_i), _p(good_w), k, _p(out_i), _p(out_s)), "k must be")
        refused(L.bert_hip_sparse_index_search_device(ix.ix, 2, 4, None, None, k, None, None, None), "k must be")
        refused(L.bert_hip_sparse_index_reserve(ix.ix, 10, 10, k), "reserve")
    for kq in (0, 257):
        refused(L.bert_hip_sparse_index_search(ix.ix, 2, kq, _p(good_i), _p(good_w), 4, _p(out_i), _p(out_s)), "kq must be")
        refused(L.bert_hip_sparse_index_search_device(ix.ix, 2, kq, None, None, 4, None, None, None), "kq must be")
    refused(L.bert_hip_sparse_index_search(ix.ix, 2, 4, None, _p(good_w), 4, _p(out_i), _p(out_s)), "pointers")
    rows_i, rows_w = np.full((2, width), 7, np.int32), np.full((2, width), 7.0, np.float32)
    for row in (-1, 70):
        refused(L.bert_hip_sparse_index_get_rows(ix.ix, 2, _p(np.array([0, row], np.int32)), _p(rows_i), _p(rows_w)), "outside")
    assert (rows_i == 7).all() and (rows_w == 7.0).all()
    with pytest.raises(ValueError):
        ix.search(good_i, good_w, 0)
    # the index is what it was
    assert _same(ix.get_rows(np.arange(70)), before)
    assert L.bert_hip_sparse_index_search(ix.ix, 0, 4, None, None, 4, None, None) == 0          # n_queries == 0: a no-op
    assert L.bert_hip_sparse_index_add(ix.ix, 0, 4, None, None) == 70
    ix.close()


def test_create_refusals_and_missing_handles(model, sparse_vocab_model, capfd):
    L = model.lib
    capfd.readouterr()
    for args, what in (((65537, 8, 1), "65536"), ((262145, 8, 0), "n_vocab"), ((-1, 8, 0), "n_vocab"), ((100, 0, 0), "width"), ((100, 257, 0), "width"),
                       ((100, 8, 2), "dtype"), ((100, 8, -1), "dtype")):
        assert not L.bert_hip_sparse_index_create(model.ctx, *args)
        assert what in capfd.readouterr().err, args
    ok = model.sparse_index(256, "f32", n_vocab=262144)
    assert ok.n_vocab == 262144
    ok.close()
    ok = model.sparse_index()
    assert ok.n_vocab == model.n_vocab                                                          # n_vocab 0: the model's
    ok.close()
    buf = np.zeros((1, 4), np.int32)
    assert L.bert_hip_sparse_index_add(None, 1, 4, _p(buf), _p(buf)) == -1 and L.bert_hip_sparse_index_size(None) == -1
    assert "no index" in capfd.readouterr().err
    tok = pybert.BertModel(sparse_vocab_model, tokenizer_only=True)
    assert not L.bert_hip_sparse_index_create(tok.ctx, 0, 8, 0)
    assert "tokenizer-only" in capfd.readouterr().err
    tok.close()


def test_bert_free_frees_the_indexes_left_alive(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    ix = m.sparse_index(8, "f16", n_vocab=100)
    ix.add(np.array([[1, 2]], np.int32), np.ones((1, 2), np.float32))
    m.close()
    ix.close()                                                   # (the context freed it: the binding must not free it again)


# ------------------------------------------------------------------------------------------------
# 5. hostile device input
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_forms_count_bad_ids_as_unused_and_stay_in_bounds(model, hip, dtype):
    rng = np.random.default_rng(23)
    V, width, rows, kq, nq, k, G = 1000, 16, 130, 16, 9, 20, 256
    ids, w = _terms(rng, rows, width, V, width, 2.0)
    q_ids, q_w = _terms(rng, nq, kq, V, kq, 2.0)
    # ids the host forms would refuse, in used and unused places, with weights that would matter
    for arr in (ids, q_ids):
        flat = arr.reshape(-1)
        for j, bad in zip(rng.permutation(flat.size)[:40], np.resize([V, V + 1, -2, -7, 2 ** 31 - 1, -2 ** 31, 65536, 262144, 1 << 20], 40)):
            flat[j] = bad
    clean = lambda a: np.where((a >= 0) & (a < V), a, -1).astype(np.int32)
    st = ref.stored_rows(clean(ids), w, width, dtype)
    want = ref.search(st[0], st[1], clean(q_ids), q_w, V, k)

    def guarded(payload, dtype_):
        """a device buffer [G canaries | payload | G canaries]; returns (base, pointer to the payload, check)"""
        canary = np.full(G, 0x5A5A5A5A, np.uint32).view(dtype_)
        host = np.concatenate([canary, payload.reshape(-1), canary])
        base = hip.upload(host)
        def check(payload_unchanged):
            now = hip.download(base, host.shape, dtype_)
            assert np.array_equal(now[:G].view(np.uint32), canary.view(np.uint32)) and np.array_equal(now[-G:].view(np.uint32), canary.view(np.uint32))
            if payload_unchanged:
                assert np.array_equal(now.view(np.uint32), host.view(np.uint32))
            return now[G:-G]
        return base, base + 4 * G, check

    b_ids, p_ids, c_ids = guarded(ids, np.int32)
    b_w, p_w, c_w = guarded(w, np.float32)
    b_qi, p_qi, c_qi = guarded(q_ids, np.int32)
    b_qw, p_qw, c_qw = guarded(q_w, np.float32)
    b_oi, p_oi, c_oi = guarded(np.full((nq, k), -9, np.int32), np.int32)
    b_os, p_os, c_os = guarded(np.full((nq, k), np.nan, np.float32), np.float32)
    ix = model.sparse_index(width, dtype, n_vocab=V)
    assert ix.add_device(rows, width, p_ids, p_w) == 0
    ix.search_device(nq, kq, p_qi, p_qw, k, p_oi, p_os)
    hip.sync()
    for c in (c_ids, c_w, c_qi, c_qw):
        c(True)
    got = c_oi(False).reshape(nq, k), c_os(False).reshape(nq, k)
    assert _same(got, want)
    assert _same(ix.get_rows(np.arange(rows)), st)
    hip.free(b_ids, b_w, b_qi, b_qw, b_oi, b_os)
    ix.close()


# ------------------------------------------------------------------------------------------------
# 6. texts
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
        path = os.path.join(model_dir, f"sparse_index_text_{int(head)}.bin")
        gf.write_model(path, hp, gf.synthetic_weights(hp, 11, mlm_head=head), gf.FTYPE_F16, vocab=[v.encode() for v in vocab])
        paths.append(path)
    words = [p for p in tok_golden["sparse_vocab"].values() if p.isalpha()]
    return paths[0], paths[1], words


@pytest.mark.parametrize("dtype", DTYPES)
def test_text_routes_are_encode_sparse_fed_to_the_index(text_model, dtype):
    path, _, words = text_model
    m = pybert.BertModel(path)
    rng = np.random.default_rng(4)
    texts = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 40, size=70)] + [""]
    queries = [" ".join(rng.choice(words, size=int(n))) for n in rng.integers(1, 12, size=9)]
    width, kq, k = 48, 16, 10
    ix = m.sparse_index(width, dtype)
    assert ix.add_texts(texts[:30]) == 0 and ix.add_texts(texts[30:]) == 30 and len(ix) == len(texts)
    t_ids, t_w = m.encode_sparse(texts, width)
    assert (t_ids >= 0).sum() > len(texts)
    st = ref.stored_rows(t_ids, t_w, width, dtype)
    assert _same(ix.get_rows(np.arange(len(texts))), st)
    q_ids, q_w = m.encode_sparse(queries, kq)
    got = ix.search_texts(queries, kq, k)
    assert _same(got, ix.search(q_ids, q_w, k))
    assert _same(got, ref.search(st[0], st[1], q_ids, q_w, m.n_vocab, k))
    assert (got[1] > 0).any()
    ix.close()
    m.close()


def test_text_routes_refuse_a_model_without_the_head_or_another_vocabulary(text_model, capfd):
    with_head, without, _ = text_model
    out_i, out_s = np.full((1, 4), 7, np.int32), np.full((1, 4), 7.0, np.float32)
    txt = (C.c_char_p * 1)(b"a")
    for path, n_vocab, what in ((without, None, "no MLM head"), (with_head, 100, "n_vocab")):
        m = pybert.BertModel(path)
        ix = m.sparse_index(8, "f32", n_vocab=n_vocab)
        capfd.readouterr()
        assert m.lib.bert_hip_sparse_index_add_texts(ix.ix, 1, 1, txt) == -2
        assert what in capfd.readouterr().err
        assert m.lib.bert_hip_sparse_index_search_texts(ix.ix, 1, 1, txt, 4, 4, _p(out_i), _p(out_s)) == -2
        assert what in capfd.readouterr().err
        assert len(ix) == 0 and (out_i == 7).all() and (out_s == 7.0).all()
        ix.close()
        m.close()


# ------------------------------------------------------------------------------------------------
# 7. stream capture
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_device_and_search_device_in_one_capture(model, hip, dtype):
    rng = np.random.default_rng(31)
    V, width, kq, nq, k = 1000, 32, 16, 9, 10
    ids, w = _terms(rng, 3000, width, V, width, 2.0)
    new_ids, new_w = _terms(rng, 70, width, V, width, 2.0)
    q_ids, q_w = _terms(rng, nq, kq, V, kq, 2.0)
    eager = model.sparse_index(width, dtype, n_vocab=V)
    eager.add(ids, w)
    eager.add(new_ids, new_w)
    want = eager.search(q_ids, q_w, k)
    ix = model.sparse_index(width, dtype, n_vocab=V)
    ix.reserve(3070, nq, k)
    ix.add(ids, w)
    d = [hip.upload(a) for a in (new_ids, new_w, q_ids, q_w)]
    d_ids, d_sc = hip.nans((nq, k), np.int32), hip.nans((nq, k))
    s = hip.stream()
    first = []
    with hip.capture(s) as cap:
        first.append(model.lib.bert_hip_sparse_index_add_device(ix.ix, 70, width, d[0], d[1], s))
        first.append(model.lib.bert_hip_sparse_index_search_device(ix.ix, nq, kq, d[2], d[3], k, d_ids, d_sc, s))
    assert first == [3000, 0] and cap.status == OK and cap.graph and len(ix) == 3070
    assert (hip.download(d_ids, (nq, k), np.int32) == -1).all(), "capturing must run nothing"
    assert hip.kernel_nodes(cap.graph) == 4                      # add, query images, scan, merge
    ex = hip.instantiate(cap.graph)
    for launch in range(2):
        hip.poison(d_ids, (nq, k), np.int32)
        hip.poison(d_sc, (nq, k))
        hip.launch(ex, s)
        assert _same((hip.download(d_ids, (nq, k), np.int32), hip.download(d_sc, (nq, k))), want), launch
    assert _same(ix.search(q_ids, q_w, k), want) and _same(ix.get_rows(np.arange(3070)), eager.get_rows(np.arange(3070)))
    hip.destroy(ex, cap.graph)
    hip.destroy_stream(s)
    hip.free(*d, d_ids, d_sc)
    ix.close()
    eager.close()


# ------------------------------------------------------------------------------------------------
# 8. bert-search --sparse
# ------------------------------------------------------------------------------------------------
def test_bert_search_sparse_finds_each_line_and_agrees_with_the_binding(text_model, tmp_path):
    path, without, words = text_model
    rng = np.random.default_rng(8)
    lines = [" ".join(rng.choice(words, size=int(n), replace=False)) for n in rng.integers(3, 12, size=10)]
    assert len(set(lines)) == 10
    file = tmp_path / "lines.txt"
    file.write_text("\n".join(lines) + "\n")
    width, k = 32, 10
    exe = os.path.join(BIN, "bert-search")
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", str(width), "-k", str(k)], input="\n".join(lines) + "\nq\n",
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Loaded 10 lines." in r.stdout
    blocks = r.stdout.split("Closest texts:\n")[1:]
    assert len(blocks) == 10
    m = pybert.BertModel(path)
    ix = m.sparse_index(width, "f32")
    ix.add_texts(lines)
    ids, sc = ix.search_texts(lines, width, k)
    for i, block in enumerate(blocks):
        found = [lines.index(l.split(". ", 1)[1]) for l in block.splitlines() if l[:1].isdigit() and ". " in l]
        shown = [float(l.split(": ")[1].rstrip(")")) for l in block.splitlines() if l.startswith(" (similarity score: ")]
        want = [int(j) for j, s in zip(ids[i], sc[i]) if j >= 0 and s > 0]
        assert found == want and i in found, (i, found, want)
        assert np.allclose(shown, sc[i][:len(want)], rtol=0, atol=6e-5 + 1e-6 * np.abs(sc[i][:len(want)]).max())      # printed with 4 decimals
    ix.close()
    m.close()
    # a model without the head, and options of the dense mode, are refused
    r = subprocess.run([exe, "-m", without, "-f", str(file), "--sparse"], input="q\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "MLM head" in r.stderr
    r = subprocess.run([exe, "-m", path, "-f", str(file), "--sparse", "--i8"], input="q\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sparse goes with" in r.stderr
