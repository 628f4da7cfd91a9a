"""The probed search with an allow-list (bert_hip_index_search_probed_filtered[_device]: search.hip's index_probe_kernel<T, true>).
The contract of bert_hip.h is the test, through public calls only: query q's result has the ids and the score bits of ONE
bert_hip_index_search_filtered whose allow-list is (the rows of the nprobe lists that the centroid index returns for q, plus the
tail) AND the caller's list.  No tolerance anywhere.  The data is probe_filter_data.py's: that of test_gpu_search_probe.py with a
tail that starts at row 1500 (no multiple of 32) and spans two 1024-row chunks, and 40 removed rows."""
import ctypes as C

import numpy as np
import pytest

import probe_filter_data as pf
from index_reference import Hip, assert_same

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

DTYPES = pf.DTYPES
f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def model(make_model):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    yield m
    m.close()


@pytest.fixture(scope="module")
def data():
    return pf.make_data()


@pytest.fixture(scope="module")
def cix(model, data):
    """the centroids as an f32 index of their own: the public restatement of the centroid stage"""
    ix = model.index(dim=pf.DIM, dtype="f32")
    ix.add(data[1])
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def indexes(model, data):
    out = {dtype: pf.make_index(model, data, dtype) for dtype in DTYPES}
    yield out
    for ix in out.values():
        ix.close()


@pytest.fixture(scope="module")
def probes(cix, data):
    """nprobe -> [Q, nprobe]: the lists of each query, computed once"""
    return {nprobe: cix.search(data[2], nprobe)[0] for nprobe in (1, 3, 12)}


def test_the_layout_this_file_relies_on(indexes, probes, data):
    for dtype, ix in indexes.items():
        lists = ix.partition_lists()
        assert len(ix) == pf.SIZE and ix.n_live == pf.SIZE - 40 and (lists[:pf.N] >= 0).all() and (lists[pf.N:] == -1).all()
        lens = np.bincount(lists[:pf.N], minlength=pf.NL)
        assert lens[pf.EMPTY] == 0 and lens.max() > 512 and (lens % 32 != 0).any(), (dtype, lens)
        gone = data[4]
        assert (gone < pf.N).any() and (gone >= pf.N).any() and len(np.unique(lists[gone])) > 3
        allows = pf.allow_lists(lists, probes[1])
        assert allows["an unprobed list only"].sum() > 0 and len(allows) == 7
        assert pf.N % 32 != 0 and (pf.SIZE - pf.N) > 1024


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nprobe", [1, 3, 12])
def test_filtered_probed_search_equals_one_filtered_search_per_query(indexes, probes, data, dtype, nprobe):
    ix, queries = indexes[dtype], data[2]
    lists = ix.partition_lists()
    for name, allow in pf.allow_lists(lists, probes[1]).items():
        for k in (1, 10, 256):
            got = ix.search_probed(queries, k, nprobe, allow=allow)
            assert_same(got, pf.probed_filtered_by_filter(ix, lists, probes[nprobe], queries, k, allow), (dtype, nprobe, name, k))
            assert not np.isin(got[0], data[4]).any()                 # (no removed row)
            if name == "no row" or (name == "an unprobed list only" and nprobe == 1):
                assert (got[0] == -1).all() and np.isneginf(got[1]).all(), (dtype, nprobe, name, k)
            elif name == "a single row":
                assert np.isin(got[0], [-1, 1234]).all() and (got[0][:, 1:] == -1).all()
            elif name == "tail rows only":
                assert (got[0][got[0] >= 0] >= pf.N).all() and (got[0][:, 0] >= pf.N).all()


def call_filtered(ix, queries, nprobe, k, words, n_words, ids, sc):
    q = np.ascontiguousarray(queries, dtype=np.float32)
    return ix.lib.bert_hip_index_search_probed_filtered(ix.ix, len(q), q.ctypes.data_as(f32p), nprobe, k, None if words is None else words.ctypes.data,
                                                        n_words, ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_allow_list_is_the_probed_search_and_a_short_one_is_refused(indexes, data, dtype, capfd):
    ix, queries = indexes[dtype], data[2]
    nprobe, k = 3, 10
    ids = np.full((pf.Q, k), 12345, np.int32)
    sc = np.full((pf.Q, k), 0.5, np.float32)
    assert call_filtered(ix, queries, nprobe, k, None, 0, ids, sc) == 0                  # allow == NULL: n_words is ignored
    assert_same((ids, sc), ix.search_probed(queries, k, nprobe), (dtype, "allow = NULL"))
    words = pybert.allow_words(np.arange(pf.SIZE) % 7 == 0, pf.SIZE)
    need = (pf.SIZE + 31) // 32
    assert len(words) == need
    ids[:], sc[:] = 12345, 0.5
    capfd.readouterr()
    assert call_filtered(ix, queries, nprobe, k, words, need - 1, ids, sc) == -2
    assert "bert_hip_index_search_probed_filtered" in capfd.readouterr().err
    assert (ids == 12345).all() and (sc == 0.5).all()
    # the argument ranges are search_probed's
    for bad_nprobe, bad_k in ((0, k), (pf.NL + 1, k), (nprobe, 0), (nprobe, 257)):
        assert call_filtered(ix, queries, bad_nprobe, bad_k, words, need, ids, sc) == -2
        assert (ids == 12345).all() and (sc == 0.5).all()
    assert call_filtered(ix, queries, nprobe, k, words, need, ids, sc) == 0
    assert_same((ids, sc), ix.search_probed(queries, k, nprobe, allow=words), (dtype, "words"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_query_with_an_allow_list(indexes, cix, data, dtype):
    ix = indexes[dtype]
    bad = data[2][:3].copy()
    bad[1, 5] = np.nan
    lists = ix.partition_lists()
    allow = np.arange(pf.SIZE) % 7 == 0
    for nprobe, k in ((1, 10), (3, 256)):
        probe = cix.search(bad, nprobe)[0]
        assert (probe[1] == -1).all()                                # (the NaN query probes no list)
        got = ix.search_probed(bad, k, nprobe, allow=allow)
        assert_same(got, pf.probed_filtered_by_filter(ix, lists, probe, bad, k, allow), (dtype, "NaN query", nprobe, k))
        # (a NaN score is never returned: the float forms scan the allowed tail rows in vain, a quantized NaN query scores NaN everywhere)
        assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all() and (got[0][[0, 2], 0] >= 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_entry_point_and_independence_of_the_other_queries(indexes, data, dtype):
    ix, queries = indexes[dtype], data[2]
    nprobe, k = 3, 100
    allow = (np.arange(pf.SIZE) >= 1390) & (np.arange(pf.SIZE) < 1655)
    words = pybert.allow_words(allow, pf.SIZE)
    want = ix.search_probed(queries, k, nprobe, allow=allow)
    for q in (0, 17, 32):
        assert_same(ix.search_probed(queries[q:q + 1], k, nprobe, allow=allow), (want[0][q:q + 1], want[1][q:q + 1]), (dtype, "alone", q))
    hip = Hip()
    s = hip.stream()
    d_q, d_w, d_i, d_s = hip.upload(queries), hip.upload(words), hip.malloc(pf.Q * k * 4), hip.malloc(pf.Q * k * 4)
    ix.search_probed_device(pf.Q, d_q, nprobe, k, d_i, d_s, s, d_allow_ptr=d_w, n_words=len(words))
    assert_same((hip.download(d_i, (pf.Q, k), np.int32), hip.download(d_s, (pf.Q, k))), want, (dtype, "device entry"))
    # without a list the device form of the binding is search_probed_device
    ix.search_probed_device(pf.Q, d_q, nprobe, k, d_i, d_s, s)
    assert_same((hip.download(d_i, (pf.Q, k), np.int32), hip.download(d_s, (pf.Q, k))), ix.search_probed(queries, k, nprobe), (dtype, "device, no list"))
    hip.free(d_q, d_w, d_i, d_s)


def test_masked_probe_profile_names(make_model, data):
    path, _ = make_model("tiny", "f16", 0)
    m = pybert.BertModel(path)
    m.profile(True)
    rows, dirs, queries = data[0], data[1], data[2]
    for dtype in DTYPES:
        ix = m.index(dim=pf.DIM, dtype=dtype)
        ix.add(rows[:300])
        ix.partition(dirs)
        ix.remove([5])
        ix.search_probed(queries[:3], 5, 2)                              # removed rows alone: the unmasked kernel
        ix.search_probed(queries[:3], 5, 2, allow=np.arange(300) % 2 == 0)
        ix.close()
    rep = m.profile_report()
    for dtype in DTYPES:
        assert rep.get(f"index_probe_{dtype}", {}).get("launches", 0) == 1, sorted(rep)
        assert rep.get(f"index_probe_{dtype}_masked", {}).get("launches", 0) == 1, sorted(rep)
    m.close()
