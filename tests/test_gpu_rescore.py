"""Rescoring (bert_hip_index_rescore[_device]: search.hip's index_rescore_kernel + topk_merge_kernel) and the two-stage search
built on it (bert_hip_index_search_rescored[_device]).  The contract is the test: for distinct candidates, query q's result has
the ids and the score bits of bert_hip_index_search_filtered called with that one query and an allow-list of exactly its
candidates; and a two-stage search equals the two public calls chained by hand."""
import ctypes as C

import numpy as np
import pytest

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "i8", "b1"]
N, DIM = 1500, 72


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)


class _Hip:
    """Just enough of the HIP runtime through ctypes (the runtime libbert.so itself is linked against)."""

    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        assert self.lib.hipMemcpy(C.c_void_p(p), C.c_void_p(arr.ctypes.data), C.c_size_t(arr.nbytes), 1) == 0
        return p

    def download(self, p, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    def stream(self):
        s = C.c_void_p()
        assert self.lib.hipStreamCreate(C.byref(s)) == 0
        return s.value

    def free(self, *ps):
        for p in ps:
            self.lib.hipFree(C.c_void_p(p))


def assert_same(got, want, what=""):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.int32) != ws.view(np.int32)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[0]][:8], wi[bad[0]][:8], gs[bad[0]][:8], ws[bad[0]][:8])


def filtered_per_query(ix, queries, cand, k):
    """the yardstick: one bert_hip_index_search_filtered per query, its allow-list exactly that query's candidates"""
    ids = np.empty((len(queries), k), np.int32)
    sc = np.empty((len(queries), k), np.float32)
    for i, q in enumerate(queries):
        allow = np.zeros(len(ix), bool)
        allow[cand[i][cand[i] >= 0]] = True
        ids[i], sc[i] = (a[0] for a in ix.search(q[None], k, allow=allow))
    return ids, sc


def candidates(rng, Q, n_cand, n_rows, holes):
    """[Q, n_cand] distinct ids per query, a tenth of the entries -1 if holes"""
    cand = np.stack([rng.permutation(n_rows)[:n_cand] for _ in range(Q)]).astype(np.int32)
    if holes:
        cand[rng.random(cand.shape) < 0.1] = -1
    return cand


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(41)
    rows = unit_rows(rng, N, DIM)
    rows[100:110] = rows[100]                                        # duplicates: equal scores, the id decides
    return rows, unit_rows(rng, 33, DIM), rng.choice(N, 200, replace=False)


@pytest.fixture(scope="module")
def indexes(model, data):
    """per dtype: (an index of all rows, an index of the same rows with 200 of them removed)"""
    rows, _, gone = data
    out = {}
    for dtype in DTYPES:
        full, holed = model.index(dim=DIM, dtype=dtype), model.index(dim=DIM, dtype=dtype)
        full.add(rows)
        holed.add(rows)
        assert holed.remove(gone) == len(gone)
        out[dtype] = (full, holed)
    yield out
    for pair in out.values():
        for ix in pair:
            ix.close()


# ---- 1. the contract

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_cand,ks", [(1, (1, 3)), (31, (10, 40)), (32, (32, 256)), (33, (1, 100)), (1024, (10, 256))])
def test_rescore_equals_a_filtered_search_per_query(indexes, data, dtype, n_cand, ks):
    _, queries, _ = data
    rng = np.random.default_rng(n_cand)
    full, holed = indexes[dtype]
    for Q in (1, 33):
        plain, with_holes = candidates(rng, Q, n_cand, N, False), candidates(rng, Q, n_cand, N, True)
        for k in ks:
            assert_same(full.rescore(queries[:Q], plain, k), filtered_per_query(full, queries[:Q], plain, k), ("full", Q, k))
            # -1 entries and removed rows are skipped
            assert_same(holed.rescore(queries[:Q], with_holes, k), filtered_per_query(holed, queries[:Q], with_holes, k), ("holed", Q, k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rescore_of_nothing_and_of_repeats(indexes, data, dtype):
    rows, queries, gone = data
    full, holed = indexes[dtype]
    # only -1 entries, only removed rows: nothing to return
    for ix, cand in ((full, np.full((2, 5), -1, np.int32)), (holed, np.stack([gone[:5], gone[5:10]]).astype(np.int32))):
        ids, sc = ix.rescore(queries[:2], cand, 3)
        assert (ids == -1).all() and np.isneginf(sc).all()
    # an id that appears twice is two candidates
    one = full.rescore(queries[:1], np.array([[5, 9]], np.int32), 2)
    i5 = one[0][0].tolist().index(5)
    ids, sc = full.rescore(queries[:1], np.array([[5, 9, 5]], np.int32), 3)
    assert sorted(ids[0].tolist()) == [5, 5, 9]
    assert all(s.view(np.int32) == one[1][0, i5].view(np.int32) for i, s in zip(ids[0], sc[0]) if i == 5)


@pytest.mark.parametrize("dtype", ["f16", "b1"])
def test_rescore_rejects_ids_out_of_range_and_bad_shapes(indexes, data, dtype, capfd):
    _, queries, _ = data
    full, _ = indexes[dtype]
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    q = np.ascontiguousarray(queries[:2])
    ids = np.full((2, 4), 12345, np.int32)
    sc = np.full((2, 4), 0.5, np.float32)

    def call(cand, n_cand, k):
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        capfd.readouterr()
        r = full.lib.bert_hip_index_rescore(full.ix, 2, q.ctypes.data_as(f32p), n_cand, cand.ctypes.data_as(i32p), k,
                                            ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
        return r, capfd.readouterr().err

    for bad in (N, -2, 2 ** 31 - 1):
        cand = np.arange(8).reshape(2, 4)
        cand[1, 2] = bad
        r, err = call(cand, 4, 4)
        assert r == -2 and "bert_hip_index_rescore" in err
        assert (ids == 12345).all() and (sc == 0.5).all()
    good = np.arange(8).reshape(2, 4)
    for n_cand, k in ((0, 4), (1025, 4), (4, 0), (4, 257)):
        r, err = call(np.zeros((2, max(n_cand, 1)), np.int32), n_cand, k)
        assert r == -2 and err
        assert (ids == 12345).all() and (sc == 0.5).all()
    r, _ = call(good, 4, 4)
    assert r == 0
    assert_same((ids, sc), full.rescore(q, good, 4))
    with pytest.raises(RuntimeError):
        full.rescore(q, np.full((2, 4), N, np.int32), 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rescore_device_entry(indexes, data, dtype):
    _, queries, _ = data
    _, holed = indexes[dtype]
    rng = np.random.default_rng(3)
    Q, n_cand, k = 33, 100, 20
    cand = candidates(rng, Q, n_cand, N, True)
    want = holed.rescore(queries, cand, k)
    # the device call treats ids outside [0, size) as -1
    wild = cand.copy()
    wild[cand == -1] = rng.choice([-5, N, N + 77, 2 ** 31 - 1, -2 ** 31], int((cand == -1).sum()))
    hip = _Hip()
    s = hip.stream()
    d_q, d_c, d_i, d_s = hip.upload(queries), hip.upload(wild), hip.malloc(Q * k * 4), hip.malloc(Q * k * 4)
    holed.rescore_device(Q, d_q, n_cand, d_c, k, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), want, "device entry")
    hip.free(d_q, d_c, d_i, d_s)


# ---- 2. two-stage search

@pytest.mark.parametrize("fine_dtype", ["i8", "f16"])
def test_search_rescored_equals_the_hand_chained_calls(indexes, data, fine_dtype):
    _, queries, _ = data
    for which in (0, 1):                                             # without and with removed rows (the same in both indexes)
        coarse, fine = indexes["b1"][which], indexes[fine_dtype][which]
        for n_cand, k in ((100, 10), (256, 256), (33, 1), (1, 1)):
            cand, _ = coarse.search(queries, n_cand)
            want = fine.rescore(queries, cand, k)
            assert_same(coarse.search_rescored(fine, queries, k, n_cand), want, (which, n_cand, k))
            assert_same(coarse.search_rescored(fine, queries[:1], k, n_cand), (want[0][:1], want[1][:1]), "one query")
    # the device form
    coarse, fine = indexes["b1"][1], indexes[fine_dtype][1]
    Q, n_cand, k = len(queries), 100, 10
    want = fine.rescore(queries, coarse.search(queries, n_cand)[0], k)
    hip = _Hip()
    s = hip.stream()
    d_q, d_i, d_s = hip.upload(queries), hip.malloc(Q * k * 4), hip.malloc(Q * k * 4)
    coarse.search_rescored_device(fine, Q, d_q, n_cand, k, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, k), np.int32), hip.download(d_s, (Q, k))), want, "device form")
    hip.free(d_q, d_i, d_s)


def test_search_rescored_preconditions(model, make_model, indexes, data, capfd):
    rows, queries, _ = data
    coarse, fine = indexes["b1"][0], indexes["i8"][0]
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    q = np.ascontiguousarray(queries[:2])
    ids = np.full((2, 4), 12345, np.int32)
    sc = np.full((2, 4), 0.5, np.float32)

    def call(c, f, n_cand, k):
        capfd.readouterr()
        r = c.lib.bert_hip_index_search_rescored(c.ix, f.ix, 2, q.ctypes.data_as(f32p), n_cand, k, ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
        return r, capfd.readouterr().err

    shorter, other_dim = model.index(dim=DIM, dtype="i8"), model.index(dim=DIM + 1, dtype="i8")
    shorter.add(rows[:N - 1])
    other_dim.add(np.zeros((N, DIM + 1), np.float32))
    path, _ = make_model("tiny", "f16", 0)
    m2 = pybert.BertModel(path)
    elsewhere = m2.index(dim=DIM, dtype="i8")
    elsewhere.add(rows)
    for what, (c, f, n_cand, k) in {"size": (coarse, shorter, 4, 4), "dim": (coarse, other_dim, 4, 4), "context": (coarse, elsewhere, 4, 4),
                                    "k > n_cand": (coarse, fine, 3, 4), "n_cand > 256": (coarse, fine, 257, 4), "k = 0": (coarse, fine, 4, 0)}.items():
        r, err = call(c, f, n_cand, k)
        assert r == -2 and "bert_hip_index_search_rescored" in err, what
        assert (ids == 12345).all() and (sc == 0.5).all(), what
    r, _ = call(coarse, fine, 4, 4)
    assert r == 0
    assert_same((ids, sc), fine.rescore(q, coarse.search(q, 4)[0], 4))
    with pytest.raises(RuntimeError):
        coarse.search_rescored(shorter, q, 4, 4)
    m2.close()
    shorter.close()
    other_dim.close()


# ---- 3. profiler names

def test_rescore_profile_names(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    rng = np.random.default_rng(2)
    rows, q = unit_rows(rng, 300, 64), unit_rows(rng, 3, 64)
    for dtype in DTYPES:
        ix = m.index(dim=64, dtype=dtype)
        ix.add(rows)
        ix.rescore(q, np.arange(30, dtype=np.int32).reshape(3, 10), 5)
        ix.close()
    rep = m.profile_report()
    for dtype in DTYPES:
        assert rep.get(f"index_rescore_{dtype}", {}).get("launches", 0) >= 1, sorted(rep)
    m.close()
