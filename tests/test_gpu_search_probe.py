"""The cluster partition and the probed search (bert_hip_index_get_rows, _partition, _search_probed[_device]: search.hip's
index_export_kernel, index_probe_kernel + topk_merge_kernel).  The contracts of bert_hip.h are the tests, restated through public
calls only: the list of a row is what a k = 1 search of an f32 index of the centroids returns for get_rows(row); query q's probed
result has the ids and the score bits of one bert_hip_index_search_filtered whose allow-list holds the rows of the nprobe lists
that the centroid index returns for q, plus the tail."""
import ctypes as C

import numpy as np
import pytest

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "f16", "i8", "b1"]
N, DIM, NL, LONG = 1500, 72, 12, 5


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


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


def unit(x):
    return (x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-30)).astype(np.float32)


def assert_same(got, want, what=""):
    (gi, gs), (wi, ws) = got, want
    assert gi.shape == wi.shape and gs.shape == ws.shape, what
    bad = np.nonzero((gi != wi).any(axis=1) | (gs.view(np.int32) != ws.view(np.int32)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gi[bad[0]][:8], wi[bad[0]][:8], gs[bad[0]][:8], ws[bad[0]][:8])


@pytest.fixture(scope="module")
def data():
    """rows [N, DIM]: 600 near direction LONG, 900 spread over ten more directions, shuffled; centroids: the twelve directions,
    centroid 7 a copy of centroid 3 — every tie goes to list 3, so list 7 is empty; 33 queries; 200 more rows"""
    rng = np.random.default_rng(77)
    dirs = unit(rng.standard_normal((NL, DIM)))
    dirs[7] = dirs[3]
    of = np.concatenate([np.full(600, LONG), rng.choice([d for d in range(NL) if d not in (LONG, 7)], 900)])
    rows = unit(dirs[of] + 0.06 * rng.standard_normal((N, DIM)))[rng.permutation(N)]
    rows[100:110] = rows[100]                                        # duplicates: equal scores, the id decides
    queries = unit(dirs[rng.integers(0, NL, 33)] + 0.1 * rng.standard_normal((33, DIM)))
    more = unit(dirs[rng.integers(0, NL, 200)] + 0.06 * rng.standard_normal((200, DIM)))
    # the layout this file relies on, by a float64 assignment (no bits needed): a list of several steps of 128 and a sort, a
    # length that is no multiple of 32, an empty list
    lens = np.bincount(np.argmax(rows.astype(np.float64) @ dirs.astype(np.float64).T, axis=1), minlength=NL)
    assert lens[LONG] > 512 and lens[7] == 0 and (lens % 32 != 0).any(), lens
    return rows, dirs, queries, more


@pytest.fixture(scope="module")
def cix(model, data):
    """the centroids as an f32 index of their own: the public restatement of the centroid stage"""
    ix = model.index(dim=DIM, dtype="f32")
    ix.add(data[1])
    yield ix
    ix.close()


def make_index(model, data, dtype):
    ix = model.index(dim=DIM, dtype=dtype)
    ix.add(data[0])
    ix.partition(data[1])
    return ix


@pytest.fixture(scope="module")
def indexes(model, data):
    out = {dtype: make_index(model, data, dtype) for dtype in DTYPES}
    yield out
    for ix in out.values():
        ix.close()


def probed_by_filter(ix, cix, queries, nprobe, k):
    """the yardstick: per query one filtered search over the rows of the lists its centroid search names, and the tail"""
    lists = ix.partition_lists()
    probe, _ = cix.search(queries, nprobe)
    ids = np.empty((len(queries), k), np.int32)
    sc = np.empty((len(queries), k), np.float32)
    for i, q in enumerate(queries):
        allow = (lists == -1) | np.isin(lists, probe[i][probe[i] >= 0])
        ids[i], sc[i] = (a[0] for a in ix.search(q[None], k, allow=allow))
    return ids, sc


# ---- 1. get_rows

def restate_rows(rows, dtype):
    """the stored row as bert_hip.h states it, in NumPy f32 arithmetic"""
    if dtype == "f32":
        return rows
    if dtype == "f16":
        return rows.astype(np.float16).astype(np.float32)
    if dtype == "b1":
        return np.where(rows > 0, np.float32(1), np.float32(-1))
    scale = (np.abs(rows).max(axis=1) / np.float32(127)).astype(np.float32)
    codes = np.clip(np.rint(rows / scale[:, None]), -127, 127).astype(np.int8).astype(np.float32)      # (int8 codes: no -0)
    return codes * scale[:, None]


@pytest.mark.parametrize("dtype", DTYPES)
def test_get_rows_returns_the_stored_rows(indexes, data, dtype, capfd):
    ix, rows = indexes[dtype], data[0]
    ids = np.random.default_rng(1).permutation(N).astype(np.int32)
    got = ix.get_rows(ids)
    want = restate_rows(rows, dtype)[ids]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert ix.get_rows([]).shape == (0, DIM)
    out = np.full((3, DIM), 0.5, np.float32)
    for bad in (N, -1, 2 ** 31 - 1):
        bad_ids = np.array([0, bad, 1], np.int32)
        capfd.readouterr()
        r = ix.lib.bert_hip_index_get_rows(ix.ix, 3, bad_ids.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_float)))
        assert r == -2 and "bert_hip_index_get_rows" in capfd.readouterr().err
        assert (out == 0.5).all()


def test_get_rows_of_a_non_finite_i8_row_is_nan(model):
    ix = model.index(dim=DIM, dtype="i8")
    rows = np.ones((3, DIM), np.float32)
    rows[1, 5] = np.inf
    ix.add(rows)
    got = ix.get_rows([0, 1, 2])
    assert np.isnan(got[1]).all() and np.array_equal(got[0], got[2]) and np.isfinite(got[0]).all()
    ix.close()


# ---- 2. assignment

@pytest.mark.parametrize("dtype", DTYPES)
def test_partition_lists_are_a_k1_search_of_the_centroids(indexes, cix, dtype):
    ix = indexes[dtype]
    assert ix.n_lists == NL and np.array_equal(ix.centroids().view(np.int32), cix.get_rows(np.arange(NL)).view(np.int32))
    lists = ix.partition_lists()
    want = cix.search(ix.get_rows(np.arange(N)), 1)[0][:, 0]
    assert (want >= 0).all() and np.array_equal(lists, want)
    lens = np.bincount(lists, minlength=NL)
    assert lens[7] == 0, lens                                        # the copy loses every tie to list 3
    if dtype != "b1":                                                # (sign rows lie elsewhere: their layout is what it is)
        assert lens[LONG] > 512 and (lens % 32 != 0).any(), lens


# ---- 3., 4. the contract

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nprobe", [1, 3, 12])
def test_probed_search_equals_a_filtered_search_per_query(indexes, cix, data, dtype, nprobe):
    ix, queries = indexes[dtype], data[2]
    for k in (1, 10, 100):
        assert_same(ix.search_probed(queries, k, nprobe), probed_by_filter(ix, cix, queries, nprobe, k), (dtype, nprobe, k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_probing_every_list_is_the_search(indexes, data, dtype):
    ix, queries = indexes[dtype], data[2]
    for k in (1, 10, 256):
        assert_same(ix.search_probed(queries, k, NL), ix.search(queries, k), (dtype, k))


# ---- 5. tail

@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_added_after_partition_are_always_candidates(model, cix, data, dtype):
    rows, dirs, queries, more = data
    ix = make_index(model, data, dtype)
    assert ix.add(more) == N
    lists = ix.partition_lists()
    assert len(lists) == N + 200 and (lists[:N] >= 0).all() and (lists[N:] == -1).all()
    for nprobe, k in ((1, 10), (3, 100)):
        got = ix.search_probed(queries, k, nprobe)
        assert_same(got, probed_by_filter(ix, cix, queries, nprobe, k), ("tail", nprobe, k))
    assert (got[0] >= N).any()                                       # (tail rows are among the results)
    ix.partition(dirs)                                               # again: everything is assigned
    lists = ix.partition_lists()
    assert (lists >= 0).all() and np.array_equal(lists, make_lists_again(ix, cix))
    assert_same(ix.search_probed(queries, 10, 3), probed_by_filter(ix, cix, queries, 3, 10), "tail emptied")
    ix.close()


def make_lists_again(ix, cix):
    return cix.search(ix.get_rows(np.arange(len(ix))), 1)[0][:, 0]


# ---- 6. removed rows, compaction

@pytest.mark.parametrize("dtype", DTYPES)
def test_removed_rows_are_skipped_and_compact_keeps_the_partition(model, cix, data, dtype):
    rows, dirs, queries, more = data
    ix = make_index(model, data, dtype)
    ix.add(more[:40])                                                # (a tail that compaction has to keep a tail)
    gone = np.random.default_rng(6).choice(N + 40, 200, replace=False).astype(np.int32)
    before = ix.partition_lists()
    assert ix.remove(gone) == 200
    assert np.array_equal(ix.partition_lists(), before)              # remove changes nothing in the partition
    for nprobe, k in ((1, 10), (3, 100), (12, 256)):
        got = ix.search_probed(queries, k, nprobe)
        assert not np.isin(got[0], gone).any()
        assert_same(got, probed_by_filter(ix, cix, queries, nprobe, k), ("removed", nprobe, k))
    old = ix.compact()
    assert len(ix) == N + 40 - 200 and ix.n_lists == NL
    assert np.array_equal(ix.partition_lists(), before[old])
    for nprobe, k in ((1, 10), (3, 100)):
        assert_same(ix.search_probed(queries, k, nprobe), probed_by_filter(ix, cix, queries, nprobe, k), ("compacted", nprobe, k))
    ix.close()


# ---- 7. independence

@pytest.mark.parametrize("dtype", DTYPES)
def test_probed_result_depends_on_nothing_but_its_query(indexes, data, dtype):
    ix, queries = indexes[dtype], data[2]
    Q, nprobe = len(queries), 3
    i100, s100 = ix.search_probed(queries, 100, nprobe)
    assert_same(ix.search_probed(queries, 10, nprobe), (i100[:, :10], s100[:, :10]), "top-10 is the first 10 of top-100")
    for q in (0, 17, 32):
        assert_same(ix.search_probed(queries[q:q + 1], 100, nprobe), (i100[q:q + 1], s100[q:q + 1]), ("alone", q))
    hip = _Hip()
    s = hip.stream()
    d_q, d_i, d_s = hip.upload(queries), hip.malloc(Q * 100 * 4), hip.malloc(Q * 100 * 4)
    ix.search_probed_device(Q, d_q, nprobe, 100, d_i, d_s, s)
    assert_same((hip.download(d_i, (Q, 100), np.int32), hip.download(d_s, (Q, 100))), (i100, s100), "device entry")
    hip.free(d_q, d_i, d_s)


# ---- 8. errors

def test_probed_search_and_partition_reject_bad_arguments(model, data, capfd):
    rows, dirs, queries, _ = data
    ix = model.index(dim=DIM, dtype="i8")
    ix.add(rows)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    q = np.ascontiguousarray(queries[:2])
    ids = np.full((2, 4), 12345, np.int32)
    sc = np.full((2, 4), 0.5, np.float32)

    def probed(nprobe, k=4):
        capfd.readouterr()
        r = ix.lib.bert_hip_index_search_probed(ix.ix, 2, q.ctypes.data_as(f32p), nprobe, k, ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
        return r, capfd.readouterr().err

    def partition(n_lists, cents):
        capfd.readouterr()
        c = np.ascontiguousarray(cents, dtype=np.float32)
        r = ix.lib.bert_hip_index_partition(ix.ix, n_lists, c.ctypes.data_as(f32p))
        return r, capfd.readouterr().err

    def untouched():
        return (ids == 12345).all() and (sc == 0.5).all()

    assert ix.n_lists == 0
    r, err = probed(1)
    assert r == -2 and "no partition" in err and untouched()
    lists = np.full(N, 99, np.int32)
    assert ix.lib.bert_hip_index_partition_lists(ix.ix, lists.ctypes.data_as(i32p)) == -2 and (lists == 99).all()
    r, err = partition(65537, np.zeros((1, DIM)))
    assert r == -2 and "bert_hip_index_partition" in err and ix.n_lists == 0
    nan = dirs.copy()
    nan[4, 9] = np.nan
    r, err = partition(NL, nan)
    assert r == -2 and "finite" in err and ix.n_lists == 0
    inf = dirs.copy()
    inf[0, 0] = np.inf
    assert partition(NL, inf)[0] == -2 and ix.n_lists == 0
    assert partition(NL, dirs)[0] == 0 and ix.n_lists == NL
    for nprobe, k in ((0, 4), (13, 4), (257, 4), (-1, 4), (3, 0), (3, 257)):
        r, err = probed(nprobe, k)
        assert r == -2 and "bert_hip_index_search_probed" in err and untouched(), (nprobe, k)
    assert ix.lib.bert_hip_index_search_probed(ix.ix, 0, None, 3, 4, None, None) == 0     # no queries: nothing to do
    r, _ = probed(3)
    assert r == 0
    assert_same((ids, sc), ix.search_probed(q, 4, 3))
    # a NaN query: only empty slots on the i8 form
    bad = q.copy()
    bad[1, 3] = np.nan
    bi, bs = ix.search_probed(bad, 4, 3)
    assert (bi[1] == -1).all() and np.isneginf(bs[1]).all()
    assert_same((bi[:1], bs[:1]), ix.search_probed(q[:1], 4, 3))
    with pytest.raises(RuntimeError):
        ix.search_probed(q, 4, 13)
    assert partition(0, np.zeros((1, DIM)))[0] == 0 and ix.n_lists == 0                 # n_lists 0 drops the partition
    ids[:], sc[:] = 12345, 0.5
    assert probed(1)[0] == -2 and untouched()
    assert_same(ix.search(q, 4), ix.search(q, 4))
    ix.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_nan_query_probes_no_list_but_scans_the_tail(model, cix, data, dtype):
    rows, dirs, queries, more = data
    ix = make_index(model, data, dtype)
    ix.add(more[:7])
    bad = queries[:2].copy()
    bad[0, 0] = np.nan
    got = ix.search_probed(bad, 5, 3)
    assert_same(got, probed_by_filter(ix, cix, bad, 3, 5), "NaN query")
    assert (got[0][0] == -1).all()                                   # (NaN scores are never returned)
    ix.close()


# ---- profiler names

def test_probe_and_export_profile_names(make_model, data):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    rows, dirs, queries, _ = data
    for dtype in DTYPES:
        ix = m.index(dim=DIM, dtype=dtype)
        ix.add(rows[:300])
        ix.partition(dirs)
        ix.search_probed(queries[:3], 5, 2)
        ix.close()
    rep = m.profile_report()
    for dtype in DTYPES:
        assert rep.get(f"index_probe_{dtype}", {}).get("launches", 0) >= 1, sorted(rep)
        assert rep.get(f"index_export_{dtype}", {}).get("launches", 0) >= 1, sorted(rep)
    m.close()
