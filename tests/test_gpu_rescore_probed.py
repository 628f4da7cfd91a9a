"""The two-stage search over a partition (bert_hip_index_search_rescored_probed[_device]): the result equals the two public calls
chained by hand — coarse.search_probed(k = n_cand, nprobe, allow), then fine.rescore of those candidates — on ids and score
bits.  Coarse indexes: b1 and f16, partitioned, with a tail and removed rows (probe_filter_data.py); fine indexes: i8 and f32 of
the same rows, without a partition."""
import ctypes as C

import numpy as np
import pytest

import probe_filter_data as pf
from index_reference import Hip, assert_same

from bert_cpp_amd import pybert

pytestmark = pytest.mark.gpu

COARSE, FINE = ["b1", "f16"], ["i8", "f32"]
NPROBE = 3
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
def indexes(model, data):
    out = {dtype: pf.make_index(model, data, dtype, partitioned=dtype in COARSE) for dtype in COARSE + FINE}
    yield out
    for ix in out.values():
        ix.close()


def allow_of(with_allow):
    return (np.arange(pf.SIZE) % 3 != 0) if with_allow else None


@pytest.mark.parametrize("coarse", COARSE)
@pytest.mark.parametrize("fine", FINE)
@pytest.mark.parametrize("with_allow", [False, True])
def test_equals_probed_search_then_rescore(indexes, data, coarse, fine, with_allow):
    cx, fx, queries = indexes[coarse], indexes[fine], data[2]
    assert cx.n_lists == pf.NL and fx.n_lists == 0                    # (the fine index needs no partition)
    allow = allow_of(with_allow)
    for n_cand, k in ((1, 1), (10, 10), (100, 10), (256, 256)):
        cand, _ = cx.search_probed(queries, n_cand, NPROBE, allow=allow)
        want = fx.rescore(queries, cand, k)
        got = cx.search_rescored_probed(fx, queries, k, n_cand, NPROBE, allow=allow)
        assert_same(got, want, (coarse, fine, with_allow, n_cand, k))
        assert not np.isin(got[0], data[4]).any()
        if with_allow:
            assert (got[0][got[0] >= 0] % 3 != 0).all()               # (no disallowed row is returned)
    assert (got[0] >= pf.N).any()                                     # (tail rows are among the results)


@pytest.mark.parametrize("coarse", COARSE)
def test_device_form_equals_host_form(indexes, data, coarse):
    cx, fx, queries = indexes[coarse], indexes["i8"], data[2]
    n_cand, k = 100, 10
    hip = Hip()
    s = hip.stream()
    d_q, d_i, d_s = hip.upload(queries), hip.malloc(pf.Q * k * 4), hip.malloc(pf.Q * k * 4)
    for with_allow in (False, True):
        allow = allow_of(with_allow)
        want = cx.search_rescored_probed(fx, queries, k, n_cand, NPROBE, allow=allow)
        words = pybert.allow_words(allow, pf.SIZE) if with_allow else None
        d_w = hip.upload(words) if with_allow else 0
        cx.search_rescored_probed_device(fx, pf.Q, d_q, NPROBE, n_cand, k, d_i, d_s, s, d_allow_ptr=d_w, n_words=len(words) if with_allow else 0)
        assert_same((hip.download(d_i, (pf.Q, k), np.int32), hip.download(d_s, (pf.Q, k))), want, (coarse, "device", with_allow))
        if d_w:
            hip.free(d_w)
    hip.free(d_q, d_i, d_s)


def test_a_row_removed_in_fine_only_is_skipped(model, indexes, data):
    cx, queries = indexes["b1"], data[2]
    fx = pf.make_index(model, data, "i8", partitioned=False)
    n_cand, k = 100, 10
    before = cx.search_rescored_probed(fx, queries, k, n_cand, NPROBE)
    victims = np.unique(before[0][:, 0])                              # every query's best row
    assert (victims >= 0).all() and fx.remove(victims) == len(victims)
    got = cx.search_rescored_probed(fx, queries, k, n_cand, NPROBE)
    assert not np.isin(got[0], victims).any()
    cand, _ = cx.search_probed(queries, n_cand, NPROBE)
    assert np.isin(victims, cand).all()                               # (the coarse stage still names them)
    assert_same(got, fx.rescore(queries, cand, k), "removed in fine only")
    fx.close()


def test_bad_arguments_are_refused(model, indexes, data, capfd):
    cx, fx, queries = indexes["b1"], indexes["i8"], data[2]
    q = np.ascontiguousarray(queries[:2])
    ids = np.full((2, 4), 12345, np.int32)
    sc = np.full((2, 4), 0.5, np.float32)
    words = pybert.allow_words(np.ones(pf.SIZE, bool), pf.SIZE)

    def call(coarse, fine, nprobe, n_cand, k, w=None, n_words=0):
        capfd.readouterr()
        r = cx.lib.bert_hip_index_search_rescored_probed(coarse.ix, fine.ix, 2, q.ctypes.data_as(f32p), nprobe, n_cand, k,
                                                         None if w is None else w.ctypes.data, n_words, ids.ctypes.data_as(i32p), sc.ctypes.data_as(f32p))
        err = capfd.readouterr().err
        assert r == 0 or ((ids == 12345).all() and (sc == 0.5).all())
        return r, err

    r, err = call(fx, cx, NPROBE, 8, 4)                               # a coarse index without a partition
    assert r == -2 and "partition" in err
    assert call(cx, fx, pf.NL + 1, 8, 4)[0] == -2                     # nprobe > n_lists
    assert call(cx, fx, 0, 8, 4)[0] == -2
    assert call(cx, fx, NPROBE, 3, 4)[0] == -2                        # k > n_cand
    assert call(cx, fx, NPROBE, 257, 4)[0] == -2
    assert call(cx, fx, NPROBE, 8, 4, words, len(words) - 1)[0] == -2     # an allow-list one word short
    small = model.index(dim=pf.DIM, dtype="i8")
    small.add(data[0])
    r, err = call(cx, small, NPROBE, 8, 4)                            # unequal sizes
    assert r == -2 and "size" in err
    small.close()
    with pytest.raises(RuntimeError, match="-2"):
        fx.search_rescored_probed(cx, q, 4, 8, NPROBE)
    assert call(cx, fx, NPROBE, 8, 4, words, len(words))[0] == 0
    assert_same((ids, sc), cx.search_rescored_probed(fx, q, 4, 8, NPROBE))
